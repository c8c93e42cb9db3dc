"""Layer-by-layer CPU restatement of the iTHOR VARPretextNet's bf16 training path (set_precision('bf16'): csrc/snd_bf16.hip,
gru_bf16.hip, img_bf16.hip, dense_bf16.h, the small_linear_* kernels and the l6_dense_* route of csrc/ithor.hip, and csrc/gg.h's
BF = true instantiation everywhere else), the checker of tests/test_gpu_ithor_bf16_layers.py.  Built on tests/ithor_layers_cpu.py
in the convention of tests/acting_bf16_cpu.py.

THE RULE.  A bf16 row is the fp32 row's function with BOTH OPERANDS OF EVERY PRODUCT rounded to bf16 before the product (`q`,
convstack_bf16_cpu.bf16_round: nearest, ties to even, dense16::bf16_bits' (u + 0x7fff + ((u >> 16) & 1)) >> 16).  Bias,
activation, gates, masks, pools, the normalisation and every sum stay unrounded.  The same rounded function is evaluated in float64
(the reference) and with torch's fp32 CPU kernels (the yardstick); a product of two bf16 values is exact in fp32, so the yardstick
is fp32 summation alone and the bounds are of the fp32 path's size: MARGIN x that distance, relative to the float64 output's
largest magnitude; routing rows are exact.

THE REFERENCE NEVER ROUNDS A VALUE IT COMPUTED ITSELF: every operand the device rounds is taken from the device's own fp32 buffer
and rounded here (otherwise the two land on different sides of a bf16 boundary and one element moves by 2^-9):
  gru.fwd    per step from the device's hb[step]; the rounded copy feeds the recurrent product only, the carry z h takes the fp32
             state (gru_bf16.hip:196 writes H16 = pack2 of the fp32 state it has just stored at :195).  A copy rounded again from
             the previous bf16 copy would be the same bits (rounding is idempotent), so that fault is not distinguishable; the
             carry taking the bf16 copy is, and tests/test_ithor_bf16_layers_host.py injects it.
  gru.bwd    DH is updated in place (gru_bf16.hip:262 / :514) and no per-step dh exists, so the row is ONE block through time
             whose recurrent product term of step s takes the DEVICE'S OWN dgh of step s + 1, rounded (gru_bf16.hip:220 / :446
             read DG16, written at :267 / :486-488 as pack2 of the fp32 dr, dz, dn r); the carry dh z and the gate derivatives
             stay this reference's float64.
  gru.wgrad, gru.dgrad, gru.input   from the device's dgi, dgh, hb, s3 (gru_bf16_convert_x / gru_bf16_to_bf16: to_bf16_kernel,
             gru_bf16.hip:552; i16 / g16 at :264-268 and :509-511); b_ih / b_hh are sums of the UNROUNDED gate gradients
             (the register sums of gru_bf16.hip:490-493 folded at :518-541 and by slab_reduce over the 64-clip slices,
             ithor.hip:1044-1048; chan_sum in the per-step form, ithor.hip:1051-1052).  The fp32 gate gradients of the sequence
             form are written only with keep_fp32_activations (store32, gru_bf16.hip:503).
  sound convolutions   from the fp32 s1 / s2 / gs1 / gs2 copies of keep_fp32_activations (snd_bf16.hip rounds in its C8 image
             writes); the bias gradients of conv 1 and conv 2 are sums of the unrounded values the data-gradient store wrote
             (ithor.hip:1083, :1104), conv 3's is chan_sum of gs3 (ithor.hip:1076).
  image layers   from a* / p* / ga* / gp* (img_bf16.hip rounds in its LDS write; gg.h:156-166 rounds with v_cvt_pk_bf16_f32 on
             the way from the fp32 LDS tile into the MFMA; l6_expand_kernel, ithor.hip:703, and gru_bf16_to_bf16 of p5 / ga6,
             ithor.hip:717 / :737).  Conv 1: the float image formed in fp32 ((float)u8 / 255.f, gg.h:277 / :440,
             img_bf16.hip:448) and then rounded.  Its bias gradient: the channel sums of the unrounded ga1 (ithor.hip:949).
  heads      bf16r on both operands in the small linears (ithor.hip:560, :579-581, :598-600); their bias sums add the unrounded
             dY (ithor.hip:579 `gs += g[u]`); the split-K dense route rounds in dense_bf16.h's staging, its finish pass
             (gg_finish_kernel) adds the slabs and the bias unrounded.

`chain` is torch standing in for the device (the host test's fault injection): stage by stage in the parameters' dtype, each
stage from the buffers before it; `rerun` recomputes what lies behind a changed buffer.  ORDER: rows measured on the MI355X
beyond MARGIN x torch's distance, whose yardstick is an fp32 emulation of the kernel's own accumulation order on the rounded
operands (never the device's output); DESIGN section 8 holds the figures."""
import torch
import torch.nn.functional as F

from tests import ithor_layers_cpu as lc
from tests.convstack_bf16_cpu import bf16_round
from tests.ithor_layers_cpu import MARGIN, layer_eval, ratio, rel, scale  # noqa: F401
from tests.ithor_layers_cpu import GH, IMG, RNN, SND, T


def ident(t):
    """Rounding switched off."""
    return t


# ---- the rows' functions: lc's, on rounded product operands -------------------------------------------------------------------
def conv_fwd(x, w, c, geo, seq=False, q=bf16_round):
    return lc.conv_fwd(q(x), q(w), c, geo, seq)


def image_input(image, like, q=bf16_round):
    """The float image in fp32 first ((float)u8 / 255.f), then the rounding, then like's dtype."""
    if q is ident:
        return lc.image_input(image, like)
    return q(lc.image_input(image, torch.empty(0, dtype=torch.float32))).to(like.dtype)


def conv1_fwd(image, w, c, q=bf16_round):
    return lc.conv_fwd(image_input(image, w, q), q(w), c, "i")


def conv_dgrad(gy, w, geo, in_shape, mask=None, seq=False, q=bf16_round):
    return lc.conv_dgrad(q(gy), q(w), geo, in_shape, mask, seq)


def conv_wgrad(x, gy, geo, w_shape, seq=False, q=bf16_round):
    return lc.conv_wgrad(q(x), q(gy), geo, w_shape, seq)


def conv1_wgrad(image, gy, w_shape, q=bf16_round):
    return lc.conv_wgrad(image_input(image, gy, q), q(gy), "i", w_shape)


def linear_fwd(x, w, c, relu, q=bf16_round):
    return lc.linear_fwd(q(x), q(w), c, relu)


def linear_bwd(x, w, dy, mask=None, q=bf16_round):
    """dW and dX from the rounded dy, db from the unrounded one."""
    dx = q(dy) @ q(w)
    return q(dy).t() @ q(x), dy.sum(0), dx if mask is None else lc.relu_mask(dx, mask)


def _gates(h, gs, w_hh, b_hh, q):
    gh = q(h) @ q(w_hh)[:, None].transpose(-1, -2) + b_hh[:, None, None, :]
    r = torch.sigmoid(gs[..., :GH] + gh[..., :GH])
    z = torch.sigmoid(gs[..., GH:2 * GH] + gh[..., GH:2 * GH])
    ghn = gh[..., 2 * GH:]
    n = torch.tanh(gs[..., 2 * GH:] + r * ghn)
    return r, z, n, ghn


def gru_fwd(hb, gi, w_hh, b_hh, q=bf16_round, carry=ident):
    """lc.gru_fwd with the recurrent product on q(h); the carry z h takes the fp32 state (`carry`: the injected fault)."""
    h = hb[:, :T]
    _, z, n, _ = _gates(h, lc.by_step(gi), w_hh, b_hh, q)
    return (1 - z) * n + z * carry(h)


def gru_bwd(gsraw, hb, gi, w_hh, b_hh, dgh_dev=None, q=bf16_round, w_back=None, nxt=None):
    """lc.gru_bwd with rounded product operands.  dgh_dev: the device's dgh, whose step s + 1 (rounded) feeds step s's recurrent
    product term instead of this function's own (None: its own, the stand-in's chain).  w_back, nxt: injected faults (the matrix
    of the backward product; step -> the step whose dgh it takes)."""
    h = hb[:, :T]
    r, z, n, ghn = _gates(h, lc.by_step(gi), w_hh, b_hh, q)
    wb = q(w_hh if w_back is None else w_back)
    dh = torch.stack([gsraw[:, :GH], gsraw[:, GH:]])
    dgs, dgh = torch.empty_like(lc.by_step(gi)), torch.empty_like(lc.by_step(gi))
    for s in range(T - 1, -1, -1):
        if s < T - 1:
            u = s + 1 if nxt is None else nxt(s)
            dh = dh + q(dgh[:, u] if dgh_dev is None else dgh_dev[:, u]) @ wb
        dn = dh * (1 - z[:, s]) * (1 - n[:, s] * n[:, s])
        dz = dh * (h[:, s] - n[:, s]) * z[:, s] * (1 - z[:, s])
        dr = dn * ghn[:, s] * r[:, s] * (1 - r[:, s])
        dgs[:, s] = torch.cat([dr, dz, dn], -1)
        dgh[:, s] = torch.cat([dr, dz, dn * r[:, s]], -1)
        dh = dh * z[:, s]
    return lc.by_time(dgs), dgh


def gru_wgrad(dgi, dgh, hb, s3, q=bf16_round):
    dw_ih, dw_hh, _, _ = lc.gru_wgrad(q(dgi), q(dgh), q(hb), q(s3))
    return dw_ih, dw_hh, dgi.sum((1, 2)), dgh.sum((1, 2))


def gru_dx(dgi, w_ih, s3, q=bf16_round):
    return lc.gru_dx(q(dgi), q(w_ih), s3)


def gru_input(s3, w_ih, b_ih, q=bf16_round):
    return lc.gru_input(q(s3), q(w_ih), b_ih)


def gru_unroll(gi, w_hh, b_hh, q=bf16_round, qh=None, carry=ident):
    """hb from h_0 = 0 (the stand-in's forward); qh: the rounding of h alone (the injected fault of a state left unrounded);
    carry: what the carry z h does to h (the injected fault of a carry that takes the bf16 copy)."""
    gs = lc.by_step(gi)
    hb = [torch.zeros(2, gi.shape[1], GH, dtype=gi.dtype)]
    qh = q if qh is None else qh
    for s in range(T):
        h = hb[-1][:, None]
        gh = qh(h) @ q(w_hh)[:, None].transpose(-1, -2) + b_hh[:, None, None, :]
        g = gs[:, s:s + 1]
        r = torch.sigmoid(g[..., :GH] + gh[..., :GH])
        z = torch.sigmoid(g[..., GH:2 * GH] + gh[..., GH:2 * GH])
        n = torch.tanh(g[..., 2 * GH:] + r * gh[..., 2 * GH:])
        hb.append(((1 - z) * n + z * carry(h))[:, 0])
    return torch.stack(hb, 1)


# ---- the single-layer checks over a dict of buffers ----------------------------------------------------------------------------
def layer_table(b, P, q=bf16_round, teacher=None):
    """lc.layer_table's rows (same names, kinds and row shape) with the rounded functions.  teacher: gru.bwd's recurrent term from
    b's own dgh (default: whenever q rounds)."""
    teacher = q is not ident if teacher is None else teacher
    rows = []

    def add(name, kind, fn, inputs, outputs):
        keys = [k for k in inputs + outputs if isinstance(k, str)]
        if all(k in b or k in P for k in keys):
            get = lambda k: (b[k] if k in b else P[k]) if isinstance(k, str) else k      # noqa: E731
            rows.append((name, kind, fn, [get(k) for k in inputs], [get(k) for k in outputs]))

    gW = lambda name: "G." + name      # noqa: E731
    add("conv1.fwd", "conv fwd", lambda x, w, c: conv1_fwd(x, w, c, q), ["image", IMG[0] + ".weight", IMG[0] + ".bias"], ["a1"])
    for l in range(2, 7):
        x = "a1" if l == 2 else f"p{l - 1}"
        geo = "i6" if l == 6 else "i"
        flat = (lambda y: y.flatten(1)) if l == 6 else (lambda y: y)
        add(f"conv{l}.fwd", "conv fwd", lambda x, w, c, geo=geo, flat=flat: flat(conv_fwd(x, w, c, geo, q=q)),
            [x, IMG[l - 1] + ".weight", IMG[l - 1] + ".bias"], [f"a{l}"])
        if l < 6:
            add(f"pool{l}.fwd", "pool fwd", lc.pool_fwd, [f"a{l}"], [f"p{l}"])
            add(f"pool{l}.bwd", "pool+relu bwd", lc.pool_relu_bwd, [f"a{l}", f"gp{l}"], [f"ga{l}"])
    add("img_head0.fwd", "linear fwd", lambda x, w, c: linear_fwd(x, w, c, True, q),
        ["a6", "imgTriplet.0.weight", "imgTriplet.0.bias"], ["hid_i"])
    add("img_head2.fwd", "linear fwd", lambda x, w, c: linear_fwd(x, w, c, False, q),
        ["hid_i", "imgTriplet.2.weight", "imgTriplet.2.bias"], ["raw_i"])
    add("img_l2norm.fwd", "l2norm fwd", lc.l2norm_fwd, ["raw_i"], ["emb_i"])
    add("img_l2norm.bwd", "l2norm bwd", lc.l2norm_bwd, ["raw_i", "gemb_i"], ["graw_i"])
    add("img_head2.bwd", "linear bwd", lambda x, w, dy: linear_bwd(x, w, dy, x, q), ["hid_i", "imgTriplet.2.weight", "graw_i"],
        [gW("imgTriplet.2.weight"), gW("imgTriplet.2.bias"), "ghid_i"])
    add("img_head0.bwd", "linear bwd", lambda x, w, dy: linear_bwd(x, w, dy, x, q), ["a6", "imgTriplet.0.weight", "ghid_i"],
        [gW("imgTriplet.0.weight"), gW("imgTriplet.0.bias"), "ga6"])
    for l in range(6, 0, -1):
        w = IMG[l - 1] + ".weight"
        geo = "i6" if l == 6 else "i"
        x = "image" if l == 1 else ("a1" if l == 2 else f"p{l - 1}")
        m = (lambda g: g.reshape(-1, 128, 3, 3)) if l == 6 else (lambda g: g)
        wshape = tuple(P[w].shape)
        if l == 1:
            add("conv1.wgrad", "conv wgrad", lambda x, g, s=wshape: conv1_wgrad(x, g, s, q), [x, "ga1"], [gW(w)])
        else:
            add(f"conv{l}.wgrad", "conv wgrad", lambda x, g, geo=geo, s=wshape, m=m: conv_wgrad(x, m(g), geo, s, q=q),
                [x, f"ga{l}"], [gW(w)])
        add(f"conv{l}.bgrad", "conv bgrad", lambda g, m=m: lc.conv_bgrad(m(g)), [f"ga{l}"], [gW(IMG[l - 1] + ".bias")])
        if l == 2:
            add("conv2.dgrad", "conv dgrad", lambda g, w, a: conv_dgrad(g, w, "i", a.shape, mask=a, q=q), ["ga2", w, "a1"], ["ga1"])
        elif l > 2:
            add(f"conv{l}.dgrad", "conv dgrad", lambda g, w, x, geo=geo, m=m: conv_dgrad(m(g), w, geo, x.shape, q=q),
                [f"ga{l}", w, x], [f"gp{l - 1}"])
    for l in (1, 2, 3):
        x = "snd" if l == 1 else f"s{l - 1}"
        w, c = SND[l - 1] + ".weight", SND[l - 1] + ".bias"
        seq, geo, wshape = l == 3, f"s{l}", tuple(P[w].shape)
        add(f"snd{l}.fwd", "conv fwd", lambda x, w, c, geo=geo, seq=seq: conv_fwd(x, w, c, geo, seq, q), [x, w, c], [f"s{l}"])
        add(f"snd{l}.wgrad", "conv wgrad", lambda x, g, geo=geo, s=wshape, seq=seq: conv_wgrad(x, g, geo, s, seq, q),
            [x, f"gs{l}"], [gW(w)])
        add(f"snd{l}.bgrad", "conv bgrad", lambda g, seq=seq: lc.conv_bgrad(g, seq), [f"gs{l}"], [gW(c)])
        if l > 1:
            add(f"snd{l}.dgrad", "conv dgrad",
                lambda g, w, x, geo=geo, seq=seq: conv_dgrad(g, w, geo, x.shape, mask=x, seq=seq, q=q), [f"gs{l}", w, x], [f"gs{l - 1}"])
    if all(f"rnn.weight_ih_l0{r}" in P for r in RNN):
        w_ih, w_hh, b_ih, b_hh = lc.rnn_params(P)
        gk = [gW(f"rnn.{k}_l0{r}") for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for r in RNN]
        add("gru.input", "linear fwd", lambda x, w, c: gru_input(x, w, c, q), ["s3", w_ih, b_ih], ["gi"])
        add("gru.fwd", "gru step fwd", lambda hb, gi, w, c: gru_fwd(hb, gi, w, c, q), ["hb", "gi", w_hh, b_hh],
            [lambda: b["hb"][:, 1:]] if "hb" in b else ["hb"])
        add("gru.concat", "gru concat", lc.gru_concat, ["hb"], ["sraw"])
        if teacher:
            add("gru.bwd", "gru gates bwd", lambda g, hb, gi, w, c, dgh: gru_bwd(g, hb, gi, w, c, dgh, q),
                ["gsraw", "hb", "gi", w_hh, b_hh, "dgh"], ["dgi", "dgh"])
        else:
            add("gru.bwd", "gru gates bwd", lambda g, hb, gi, w, c: gru_bwd(g, hb, gi, w, c, None, q),
                ["gsraw", "hb", "gi", w_hh, b_hh], ["dgi", "dgh"])
        if all(k in b for k in gk):
            add("gru.wgrad", "gru wgrad", lambda dgi, dgh, hb, s3: gru_wgrad(dgi, dgh, hb, s3, q), ["dgi", "dgh", "hb", "s3"],
                [torch.stack([b[gk[2 * i]], b[gk[2 * i + 1]]]) for i in range(4)])
        add("gru.dgrad", "gru dgrad", lambda dgi, w, s3: gru_dx(dgi, w, s3, q), ["dgi", w_ih, "s3"], ["gs3"])
    heads = (("snd_head0", "sraw", "soundTriplet.0", "hid_s1", "ghid_s1", "gsraw"),
             ("snd_head2", "hid_s1", "soundTriplet.2", "hid_s2", "ghid_s2", "ghid_s1"),
             ("snd_head4", "hid_s2", "soundTriplet.4", "raw_s", "graw_s", "ghid_s2"))
    for name, x, lin, y, gy, gx in heads:
        relu, masked = y != "raw_s", x != "sraw"
        add(name + ".fwd", "linear fwd", lambda x, w, c, relu=relu: linear_fwd(x, w, c, relu, q), [x, lin + ".weight", lin + ".bias"], [y])
        add(name + ".bwd", "linear bwd", lambda x, w, dy, masked=masked: linear_bwd(x, w, dy, x if masked else None, q),
            [x, lin + ".weight", gy], [gW(lin + ".weight"), gW(lin + ".bias"), gx])
    add("snd_l2norm.fwd", "l2norm fwd", lc.l2norm_fwd, ["raw_s"], ["emb_s"])
    add("snd_l2norm.bwd", "l2norm bwd", lc.l2norm_bwd, ["raw_s", "gemb_s"], ["graw_s"])
    return [(n, k, f, i, [o() if callable(o) else o for o in outs]) for n, k, f, i, outs in rows]


# ---- the kernels' own accumulation orders ---------------------------------------------------------------------------------------
def chunk_dot(A, B, chunk=16):
    """A (M, K) @ B (K, N) on ONE fp32 accumulator per output, k in order, `chunk` products per v_mfma_f32_32x32x16_bf16: the
    products of bf16 values are exact; the 16 of one instruction are taken as summed exactly and added to the accumulator with
    one rounding -- the tightest model of an instruction whose inner order is not documented (any order of rounded additions
    inside it only adds error), so this yardstick is never wider than the kernel's own order makes it."""
    A, B = A.double(), B.double()
    acc = torch.zeros(A.shape[0], B.shape[1], dtype=torch.float32)
    for k in range(0, A.shape[1], chunk):
        acc = (acc.double() + A[:, k:k + chunk] @ B[k:k + chunk]).float()
    return acc


def snd2_fwd_order(x, w, c):
    """snd_fwd_kernel (snd_bf16.hip:228-268): one accumulator per output over 4 quarters of 16 input channels x the 55 taps in
    (ky, kx) order, 16 channels per instruction.  First and last clip, over the whole output's magnitude."""
    clips = [0, x.shape[0] - 1]
    xr, wr = bf16_round(x[clips].float()), bf16_round(w.float())
    cols = F.unfold(xr, (11, 5), padding=(5, 5), stride=2)                           # (n, (ci, tap), pixels)
    n, _, pix = cols.shape
    cols = cols.view(n, 4, 16, 55, pix).permute(1, 3, 2, 0, 4).reshape(4 * 55 * 16, n * pix)      # k = (quarter, tap, ci of 16)
    wm = wr.view(64, 4, 16, 55).permute(0, 1, 3, 2).reshape(64, -1)
    y = F.relu(chunk_dot(wm, cols) + c.float()[:, None])
    return {0: (clips, y.view(64, n, 150, 13).transpose(0, 1))}


def conv6_dgrad_order(g, w, x):
    """The gather-GEMM's stride-2 data gradient below 64 images (gg.h ConvDgradS2P on gg_kernel<.., BF = true>, gg.h:149-171): the
    input pixels in four parity classes, k = (co, i, j) over the taps ky = ry + 2 i, kx = rx + 2 j of the class, one accumulator,
    16 k per instruction (taps that fall outside the map are zeros inside their chunk)."""
    g, w = bf16_round(g.float().reshape(-1, 128, 3, 3)), bf16_round(w.float())
    n, _, H, W = x.shape
    out = torch.zeros(n, 128, H, W)
    gp = F.pad(g, (1, 1, 1, 1))
    for cy in range(2):
        for cx in range(2):
            kys, kxs = range((cy + 1) % 2, 3, 2), range((cx + 1) % 2, 3, 2)
            ys, xs = torch.arange(cy, H, 2), torch.arange(cx, W, 2)
            if len(ys) == 0 or len(xs) == 0:
                continue
            A = torch.stack([gp[:, :, ((ys + 1 - ky) // 2 + 1).clamp(0, 4)][:, :, :, ((xs + 1 - kx) // 2 + 1).clamp(0, 4)]
                             for ky in kys for kx in kxs], 2)                        # (n, co, taps, ny, nx)
            Bm = torch.stack([w[:, :, ky, kx] for ky in kys for kx in kxs], 1)       # (co, taps, ci)
            r = chunk_dot(A.permute(0, 3, 4, 1, 2).reshape(-1, 128 * A.shape[2]), Bm.reshape(-1, 128))
            out[:, :, cy::2, cx::2] = r.view(n, len(ys), len(xs), 128).permute(0, 3, 1, 2)
    return {0: (slice(None), out)}


def _bias_seq(d):
    """(dir, step, clip, 1536) -> (dir, 1536) as gru_seq_bwd_kernel sums it (gru_bf16.hip:490-493, :518-541): per clip one
    accumulator over the steps, last step first; the 8 clips of a wave by lane exchange (xor 8, 16, 32: a tree); the 8 waves of
    the 64-clip slice in order; the slices in order (slab_reduce, ithor.hip:1047-1048).  Clips past the last add zeros."""
    dirs, steps, n, g = d.shape
    acc = torch.zeros(dirs, n, g)
    for s in range(steps - 1, -1, -1):
        acc = acc + d[:, s]
    v = torch.cat([acc, torch.zeros(dirs, (-n) % 64, g)], 1).view(dirs, -1, 8, 8, g)              # (slice, wave, clip of the wave)
    for _ in range(3):
        v = v[:, :, :, 0::2] + v[:, :, :, 1::2]
    v = v[:, :, :, 0]
    t = v[:, :, 0]
    for wave in range(1, 8):
        t = t + v[:, :, wave]
    out = t[:, 0]
    for sl in range(1, t.shape[1]):
        out = out + t[:, sl]
    return out


def gru_bias_order(dgi, dgh, hb, s3):
    return {2: (slice(None), _bias_seq(lc.by_step(dgi.float()))), 3: (slice(None), _bias_seq(dgh.float()))}


# Rows measured on the MI355X beyond MARGIN x torch's fp32 distance on the rounded operands (figures and reasons: DESIGN section
# 8): {name: inputs -> {output index: (index into that output, fp32 emulation of the kernel's own accumulation order on the
# ROUNDED operands)}}; the emulation's distance from float64, over the whole output's largest magnitude, replaces torch's for
# that output.  Each emulation is one route's order: order_for picks the entries of the routes that ran.
ORDER = {"snd2.fwd": snd2_fwd_order, "conv6.dgrad": conv6_dgrad_order, "gru.wgrad": gru_bias_order}


def order_for(B, sequence):
    """ORDER's entries for a step of B images: conv 6's data gradient is the gather-GEMM's below 64 images (l6_dense_dgrad from
    64 on, ithor.hip:714); the GRU's bias sums are the sequence kernel's only when each pass is one launch."""
    return {k: v for k, v in ORDER.items() if (k != "conv6.dgrad" or B < 64) and (k != "gru.wgrad" or sequence)}


def check_layers(b, P, only=None, log=None, q=bf16_round, teacher=None, order=None):
    """lc.check_layers over layer_table(b, P, q): {name: (kind, [(error, distance, ratio)] per output)}; order: as ORDER (default:
    all of it)."""
    out = {}
    order = ORDER if order is None else order
    for name, kind, fn, inputs, outputs in layer_table(b, P, q, teacher):
        if only is not None and not only(name):
            continue
        ref, dist = layer_eval(fn, inputs)
        if name in order:
            dist = list(dist)
            for i, (idx, emu) in order[name](*inputs).items():
                dist[i] = rel(emu, ref[i][idx], scale(ref[i]))
        res = [(rel(got, r), d, ratio(rel(got, r), d)) for got, r, d in zip(outputs, ref, dist)]
        out[name] = (kind, res)
        if log:
            log(f"{name:16s} {kind:14s} " + "  ".join(f"err {e:.2e} dist {d:.2e} ratio {x:.2f}" for e, d, x in res))
    return out


# ---- torch standing in for the device -----------------------------------------------------------------------------------------
def stages(P, image, snd, gemb_i, gemb_s, q=bf16_round):
    """[(outputs, inputs, fn)] in execution order: the rounded model as a chain of the row functions in P's dtype; a stage's fn
    maps its input buffers to its output buffers."""
    dt = P["cnn.0.weight"].dtype
    S = []
    add = lambda outs, ins, fn: S.append((tuple(outs), tuple(ins), fn))      # noqa: E731
    p = lambda k: P[k]      # noqa: E731
    if image is not None:
        add(["a1"], [], lambda: conv1_fwd(image, p(IMG[0] + ".weight"), p(IMG[0] + ".bias"), q))
        add(["a2"], ["a1"], lambda x: conv_fwd(x, p(IMG[1] + ".weight"), p(IMG[1] + ".bias"), "i", q=q))
        for l in range(2, 6):
            add([f"p{l}"], [f"a{l}"], lc.pool_fwd)
            add([f"a{l + 1}"], [f"p{l}"], lambda x, l=l: (lambda y: y.flatten(1) if l == 5 else y)(
                conv_fwd(x, p(IMG[l] + ".weight"), p(IMG[l] + ".bias"), "i6" if l == 5 else "i", q=q)))
        add(["hid_i"], ["a6"], lambda x: linear_fwd(x, p("imgTriplet.0.weight"), p("imgTriplet.0.bias"), True, q))
        add(["raw_i"], ["hid_i"], lambda x: linear_fwd(x, p("imgTriplet.2.weight"), p("imgTriplet.2.bias"), False, q))
        add(["emb_i"], ["raw_i"], lc.l2norm_fwd)
    if snd is not None:
        w_ih, w_hh, b_ih, b_hh = lc.rnn_params(P)
        add(["s1"], [], lambda: conv_fwd(snd.to(dt), p("cnn.0.weight"), p("cnn.0.bias"), "s1", q=q))
        add(["s2"], ["s1"], lambda x: conv_fwd(x, p("cnn.2.weight"), p("cnn.2.bias"), "s2", q=q))
        add(["s3"], ["s2"], lambda x: conv_fwd(x, p("cnn.4.weight"), p("cnn.4.bias"), "s3", True, q))
        add(["gi"], ["s3"], lambda x: gru_input(x, w_ih, b_ih, q))
        add(["hb"], ["gi"], lambda gi: gru_unroll(gi, w_hh, b_hh, q))
        add(["sraw"], ["hb"], lc.gru_concat)
        add(["hid_s1"], ["sraw"], lambda x: linear_fwd(x, p("soundTriplet.0.weight"), p("soundTriplet.0.bias"), True, q))
        add(["hid_s2"], ["hid_s1"], lambda x: linear_fwd(x, p("soundTriplet.2.weight"), p("soundTriplet.2.bias"), True, q))
        add(["raw_s"], ["hid_s2"], lambda x: linear_fwd(x, p("soundTriplet.4.weight"), p("soundTriplet.4.bias"), False, q))
        add(["emb_s"], ["raw_s"], lc.l2norm_fwd)
    if image is not None and gemb_i is not None:
        add(["graw_i"], ["raw_i"], lambda r: lc.l2norm_bwd(r, gemb_i.to(dt)))
        add(["G.imgTriplet.2.weight", "G.imgTriplet.2.bias", "ghid_i"], ["hid_i", "graw_i"],
            lambda x, dy: linear_bwd(x, p("imgTriplet.2.weight"), dy, x, q))
        add(["G.imgTriplet.0.weight", "G.imgTriplet.0.bias", "ga6"], ["a6", "ghid_i"],
            lambda x, dy: linear_bwd(x, p("imgTriplet.0.weight"), dy, x, q))
        for l in range(6, 0, -1):
            wk, geo = IMG[l - 1] + ".weight", "i6" if l == 6 else "i"
            xk = None if l == 1 else ("a1" if l == 2 else f"p{l - 1}")
            m = (lambda g: g.reshape(-1, 128, 3, 3)) if l == 6 else (lambda g: g)
            if l == 1:
                add(["G." + wk], ["ga1"], lambda g, wk=wk: conv1_wgrad(image, g, p(wk).shape, q))
            else:
                add(["G." + wk], [xk, f"ga{l}"], lambda x, g, wk=wk, geo=geo, m=m: conv_wgrad(x, m(g), geo, p(wk).shape, q=q))
            add([f"G.{IMG[l - 1]}.bias"], [f"ga{l}"], lambda g, m=m: lc.conv_bgrad(m(g)))
            if l == 2:
                add(["ga1"], ["ga2", "a1"], lambda g, a, wk=wk: conv_dgrad(g, p(wk), "i", a.shape, mask=a, q=q))
            elif l > 2:
                add([f"gp{l - 1}"], [f"ga{l}", xk], lambda g, x, wk=wk, geo=geo, m=m: conv_dgrad(m(g), p(wk), geo, x.shape, q=q))
                add([f"ga{l - 1}"], [f"a{l - 1}", f"gp{l - 1}"], lc.pool_relu_bwd)
    if snd is not None and gemb_s is not None:
        add(["graw_s"], ["raw_s"], lambda r: lc.l2norm_bwd(r, gemb_s.to(dt)))
        add(["G.soundTriplet.4.weight", "G.soundTriplet.4.bias", "ghid_s2"], ["hid_s2", "graw_s"],
            lambda x, dy: linear_bwd(x, p("soundTriplet.4.weight"), dy, x, q))
        add(["G.soundTriplet.2.weight", "G.soundTriplet.2.bias", "ghid_s1"], ["hid_s1", "ghid_s2"],
            lambda x, dy: linear_bwd(x, p("soundTriplet.2.weight"), dy, x, q))
        add(["G.soundTriplet.0.weight", "G.soundTriplet.0.bias", "gsraw"], ["sraw", "ghid_s1"],
            lambda x, dy: linear_bwd(x, p("soundTriplet.0.weight"), dy, None, q))
        add(["dgi", "dgh"], ["gsraw", "hb", "gi"], lambda g, hb, gi: gru_bwd(g, hb, gi, w_hh, b_hh, None, q))
        gk = [f"G.rnn.{k}_l0{r}" for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh") for r in RNN]
        add(gk, ["dgi", "dgh", "hb", "s3"], lambda *a: tuple(v[d] for v in gru_wgrad(*a, q=q) for d in range(2)))
        add(["gs3"], ["dgi", "s3"], lambda dgi, s3: gru_dx(dgi, w_ih, s3, q))
        for l in (3, 2, 1):
            wk, seq = SND[l - 1] + ".weight", l == 3
            if l == 1:
                add(["G." + wk], ["gs1"], lambda g, wk=wk: conv_wgrad(snd.to(dt), g, "s1", p(wk).shape, q=q))
            else:
                add(["G." + wk], [f"s{l - 1}", f"gs{l}"], lambda x, g, wk=wk, l=l, seq=seq: conv_wgrad(x, g, f"s{l}", p(wk).shape, seq, q))
            add([f"G.{SND[l - 1]}.bias"], [f"gs{l}"], lambda g, seq=seq: lc.conv_bgrad(g, seq))
            if l > 1:
                add([f"gs{l - 1}"], [f"gs{l}", f"s{l - 1}"],
                    lambda g, x, wk=wk, l=l, seq=seq: conv_dgrad(g, p(wk), f"s{l}", x.shape, mask=x, seq=seq, q=q))
    return S


def _inputs(image, snd, gemb_i, gemb_s, dt):
    b = {}
    if image is not None:
        b["image"] = image
        if gemb_i is not None:
            b["gemb_i"] = gemb_i.to(dt)
    if snd is not None:
        b["snd"] = snd.to(dt)
        if gemb_s is not None:
            b["gemb_s"] = gemb_s.to(dt)
    return b


def chain(P, image, snd, gemb_i=None, gemb_s=None, q=bf16_round):
    """Every buffer of the rounded model under its debug name, in P's dtype (with q = ident: lc.chain's values)."""
    b = _inputs(image, snd, gemb_i, gemb_s, P["cnn.0.weight"].dtype)
    for outs, ins, fn in stages(P, image, snd, gemb_i, gemb_s, q):
        b.update(zip(outs, lc._tuple(fn(*[b[k] for k in ins]))))
    return b


def rerun(P, image, snd, gemb_i, gemb_s, base, changed, q=bf16_round):
    """The buffers of `base` (a chain's) with `changed` ({name: faulted value}) in place and every stage behind a changed buffer
    computed again from it; (buffers, names that were recomputed or changed)."""
    b, dirty = dict(base), set(changed)
    b.update(changed)
    for outs, ins, fn in stages(P, image, snd, gemb_i, gemb_s, q):
        if dirty.intersection(ins):
            for k, v in zip(outs, lc._tuple(fn(*[b[k] for k in ins]))):
                if k not in changed:
                    b[k] = v
                    dirty.add(k)
    return b, dirty

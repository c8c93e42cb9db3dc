"""CPU-only checks of tests/kuka_layers_cpu.py, the float64 layer reference of tests/test_gpu_kuka_layers.py:
(1) chained in order, the layer functions reproduce oracle.torch_oracle.KukaNetCPU in float64 -- forward, torch.autograd backward
from dense cotangents, every intermediate map in the device's buffer layout, all 26 parameter gradients, also for an image-only
and a positive-sound-only call, and the fused head against torch's TripletMarginLoss -- to 1e-12; (2) with torch fp32 standing in
for the device every row passes its bound, and each injected fault (one dropped border tap in one output row, the last 16 k-terms
of one weight-gradient element, one image's contribution to a weight gradient, the negative clips' rows taken from the wrong
offset, one ReLU mask taken from the neighbouring image) fails EXACTLY its own row: the fault is put into the chain where the
kernel would leave it, and everything behind it is computed from the faulted buffer; a NaN is reported as inf; (3) the inputs of
the GPU cases A-E keep the fp32 stand-in's ReLU gates within the flip cap of the end-to-end check."""
import pytest
import torch
import torch.nn.functional as F

from oracle.torch_oracle import KukaNetCPU
from tests import kuka_layers_cpu as kc


def spec(h, B, seed, u8=False, neg=True):
    return dict(h=h, B=B, u8=u8, ch=3, neg=neg, seed=seed)


def oracle_net(h, seed):
    torch.manual_seed(seed)
    return KukaNetCPU(h)


@pytest.mark.parametrize("h", [84, 96])
def test_chain_reproduces_the_oracle_in_float64(h):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    net = oracle_net(h, 31).double()
    P = {k: v.detach() for k, v in net.named_parameters()}
    B = 2
    image, snd, g_i, g_s = kc.make_inputs(spec(h, B, 7 + h))
    g_i, g_s = g_i.double(), g_s.double()
    got = kc.chain(P, image.double(), snd.double(), g_i, g_s)

    ref = {}

    def keep(name):
        def hook(_m, _i, out):
            out.retain_grad()
            ref.setdefault(name, []).append(out)             # (the sound modules run twice: positive, then negative clips)
        return hook

    hooks = [net.imgBranch[2 * l + 1].register_forward_hook(keep(f"act{l + 1}")) for l in range(5)]
    hooks += [net.soundCNN[2 * l + 1].register_forward_hook(keep(f"sact{l + 1}")) for l in range(4)]
    hooks += [net.imgTriplet[1].register_forward_hook(keep("hid_i")), net.imgTriplet[2].register_forward_hook(keep("raw_i")),
              net.soundTriplet[1].register_forward_hook(keep("hid_s")), net.soundTriplet[2].register_forward_hook(keep("raw_s"))]
    emb_i, emb_p, emb_n = net(image.double(), snd[:B].double(), snd[B:].double())
    torch.autograd.backward([emb_i, emb_p, emb_n], [g_i, g_s[:B], g_s[B:]])
    for hk in hooks:
        hk.remove()

    def close(name, a, r):
        assert a.shape == r.shape, (name, a.shape, r.shape)
        e = kc.rel(a, r.detach())
        assert e <= 1e-12, (name, e)

    close("emb_i", got["emb_i"], emb_i)
    close("emb_s", got["emb_s"], torch.cat([emb_p, emb_n]))
    assert len(ref) == 13
    for k, outs in ref.items():
        r, g = torch.cat([o.detach() for o in outs]), torch.cat([o.grad for o in outs])
        close(k, got[k], r)
        # the device keeps gradients wrt PRE-activations: autograd's gradient wrt a ReLU's output, times that ReLU's gate
        # (the un-normalised embeddings have no gate); gact1 is never stored
        if k == "act1":
            continue
        gk = {"hid_i": "ghid_i", "hid_s": "ghid_s", "raw_i": "graw_i", "raw_s": "graw_s"}.get(k, "g" + k)
        close(gk, got[gk], g if k.startswith("raw") else g * (r > 0))
    grads = dict(net.named_parameters())
    assert len(grads) == 26
    for k, p in grads.items():
        close("G." + k, got["G." + k], p.grad)
    # every single-layer check holds on the chain's own buffers at float64 round-off
    table = kc.layer_table(got, P)
    assert len(table) == 48, [t[0] for t in table]
    for name, _kind, fn, ins, outs in table:
        for o, r in zip(outs, kc._tuple(fn(*ins))):
            assert kc.rel(o, r) <= 1e-12, name

    # an image-only and a positive-sound-only call: the other half's tensors do not exist
    net.zero_grad()
    F.normalize(net.imgTriplet(net.imgBranch(image.double())), p=2, dim=1).backward(g_i)
    half = kc.chain(P, image.double(), None, g_i, None)
    assert not any(k.startswith(("G.sound", "sact", "gsact")) for k in half)
    for k, p in grads.items():
        if k.startswith("img"):
            close("image-only G." + k, half["G." + k], p.grad)
    net.zero_grad()
    F.normalize(net.soundTriplet(net.soundCNN(snd[:B].double())), p=2, dim=1).backward(g_s[:B])
    half = kc.chain(P, None, snd[:B].double(), None, g_s[:B])
    assert not any(k.startswith(("G.img", "act", "gact")) for k in half)
    for k, p in grads.items():
        if k.startswith("sound"):
            close("positive-only G." + k, half["G." + k], p.grad)

    # the fused head: loss and gradients of torch's own TripletMarginLoss
    net.zero_grad()
    a, p_, n_ = net(image.double(), snd[:B].double(), snd[B:].double())
    loss = torch.nn.TripletMarginLoss(margin=1.0, p=2)(a, p_, n_)
    loss.backward()
    fz = kc.chain(P, image.double(), snd.double(), fused=(1.0, 1.0 / B))
    close("loss", fz["loss"], loss.reshape(1))
    assert float(loss.detach()) > 0
    for k, p in grads.items():
        close("fused G." + k, fz["G." + k], p.grad)
    rows = kc.layer_table(fz, P, fused=(1.0, 1.0 / B))
    row = [t for t in rows if t[0] == "fused.heads"]
    assert len(row) == 1 and not any(t[0].endswith(".bwd") for t in rows)
    for o, r in zip(row[0][4], kc._tuple(row[0][2](*row[0][3]))):
        assert kc.rel(o, r) <= 1e-12


STAND_IN = spec(84, 5, 91, u8=True)


def stand_in_params():
    return {k: v.detach() for k, v in oracle_net(84, 31).named_parameters()}


@pytest.fixture(scope="module")
def stand_in():
    """torch fp32 as the device: every buffer of a forward and backward at h = 84, B = 5 from the fp32 chain."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    P = stand_in_params()
    image, snd, g_i, g_s = kc.make_inputs(STAND_IN)
    return P, kc.chain(P, image, snd, g_i, g_s)


def worst(res, name):
    return max(q for _e, _d, q in res[name][1])


def failing(res):
    return sorted(n for n in res if not worst(res, n) <= 1)


def test_unfaulted_fp32_stand_in_passes_every_layer(stand_in):
    P, b = stand_in
    res = kc.check_layers(b, P)
    assert len(res) == 48
    assert {k for k, _ in res.values()} == {"img conv fwd", "img conv dgrad", "img conv wgrad", "img conv bgrad",
                                            "img conv2 dgrad + conv1 wgrad, bgrad", "snd conv fwd", "snd conv dgrad",
                                            "snd conv wgrad", "snd conv bgrad", "linear fwd", "linear bwd", "linear bgrad", "l2norm fwd", "l2norm bwd"}
    assert failing(res) == [], {n: res[n] for n in failing(res)}
    # and the fused step's rows
    fz = kc.chain(P, *kc.make_inputs(STAND_IN)[:2], fused=(1.0, 0.2))
    res = kc.check_layers(fz, P, fused=(1.0, 0.2))
    assert len(res) == 39 and len(res["fused.heads"][1]) == 11 and failing(res) == [], {n: res[n] for n in failing(res)}


def faulted_chain(P, fault):
    image, snd, g_i, g_s = kc.make_inputs(STAND_IN)
    return kc.chain(P, image, snd, g_i, g_s, fault=fault)


def only_row_failing(P, fault, row):
    b = faulted_chain(P, fault)
    res = kc.check_layers(b, P)
    assert failing(res) == [row], (row, {n: res[n] for n in failing(res)})


def test_a_dropped_border_tap_fails_its_own_row(stand_in):
    P, _ = stand_in

    def conv3_row0(v, b):                                          # output row 0 of one channel of one image misses tap (2, 0)
        w = P["imgBranch.4.weight"].clone()
        w[:, :, 2, 0] = 0
        v = v.clone()
        ch = int(v[1, :, 0].sum(1).argmax())
        v[1, ch, 0] = kc.conv_fwd(b["act2"], w, P["imgBranch.4.bias"], kc.IGEO)[1, ch, 0]
        return v

    def snd1_last_row(v, b):                                       # the last output row of one channel of one clip misses tap (4, 10)
        w = P["soundCNN.0.weight"].clone()
        w[:, :, 4, 10] = 0
        v = v.clone()
        ch = int(v[3, :, 47, 0].argmax())
        v[3, ch, 47] = kc.conv_fwd(b["snd"], w, P["soundCNN.0.bias"], kc.SGEO)[3, ch, 47]
        return v

    only_row_failing(P, {"act3": conv3_row0}, "conv3.fwd")
    only_row_failing(P, {"sact1": snd1_last_row}, "snd1.fwd")


def test_sixteen_missing_terms_of_one_weight_gradient_element_fail_their_own_row(stand_in):
    P, b = stand_in
    # k runs over (image | clip, oy, ox): the last 16 are the end of the last image's last rows
    for name, x, g, key, ky, kx, geo in (("conv3.wgrad", b["act2"], b["gact3"], "G.imgBranch.4.weight", 1, 1, kc.IGEO),
                                         ("snd2.wgrad", b["sact1"], b["gsact2"], "G.soundCNN.2.weight", 2, 0, kc.SGEO)):
        (sh, sw), (ph, pw) = geo
        W, xv = g.shape[-1], torch.zeros(x.shape[1], 16)
        for j, q in enumerate(range(g.shape[-2] * W - 16, g.shape[-2] * W)):
            oy, ox = divmod(q, W)
            iy, ix = oy * sh - ph + ky, ox * sw - pw + kx
            if 0 <= iy < x.shape[-2] and 0 <= ix < x.shape[-1]:
                xv[:, j] = x[-1, :, iy, ix]
        missing = g[-1].flatten(1)[:, -16:].double() @ xv.double().t()           # (co, ci): what each element loses
        co, ci = divmod(int(missing.abs().argmax()), x.shape[1])                # (many units are dead past a ReLU: a live pair)
        miss = float(missing[co, ci])
        assert miss != 0.0

        def drop(v, _b, el=(co, ci, ky, kx), miss=miss):
            v = v.clone()
            v[el] -= miss
            return v

        only_row_failing(P, {key: drop}, name)


def test_one_images_contribution_missing_from_a_weight_gradient_fails_its_own_row(stand_in):
    P, _ = stand_in
    for l, img in ((2, 4), (4, 0)):
        key = f"G.imgBranch.{2 * l - 2}.weight"
        only_row_failing(P, {key: lambda v, b, l=l, i=img: v - kc.conv_wgrad(b[f"act{l - 1}"][i:i + 1], b[f"gact{l}"][i:i + 1], kc.IGEO, v.shape)},
                         f"conv{l}.wgrad")
    only_row_failing(P, {"G.soundCNN.4.weight": lambda v, b: v - kc.conv_wgrad(b["sact2"][9:], b["gsact3"][9:], kc.SGEO, v.shape)},
                     "snd3.wgrad")
    only_row_failing(P, {"G.imgBranch.0.bias": lambda v, b: v - kc.conv1_grads(b["gact2"][2:3], P["imgBranch.2.weight"], b["act1"][2:3],
                                                                              b["image"][2:3], (32, 3, 3, 3))[1]}, "conv1.grads")


def test_negative_rows_taken_at_the_wrong_offset_fail_their_own_row(stand_in):
    """The negative clips' rows live at offset B; a kernel that looks for them at offset maxB finds the rows of a larger batch's
    plan: here zeros (a fresh workspace) or the positive clips' rows."""
    P, _ = stand_in
    B = STAND_IN["B"]

    def head2_reads_zeros(v, b):                                   # raw_s of the negative rows from a zero hid_s
        v = v.clone()
        v[B:] = P["soundTriplet.2.bias"]
        return v

    def conv3_reads_positive(v, b):                                # sact3 of the negative clips from the positive clips' sact2
        v = v.clone()
        v[B:] = v[:B]
        return v

    def head0_wgrad_reads_zeros(v, b):                             # dW0 without the negative rows' sact4
        return v - b["ghid_s"][B:].t() @ b["sact4"][B:].flatten(1)

    def dgrad_masks_with_positive(v, b):                           # gsact2's negative half masked by the positive half's sact2
        v = v.clone()
        full = torch.nn.grad.conv2d_input(tuple(b["sact2"].shape), P["soundCNN.4.weight"], b["gsact3"], stride=(2, 1))
        v[B:] = full[B:] * (b["sact2"][:B] > 0)
        return v

    only_row_failing(P, {"raw_s": head2_reads_zeros}, "snd_head2.fwd")
    only_row_failing(P, {"sact3": conv3_reads_positive}, "snd3.fwd")
    only_row_failing(P, {"G.soundTriplet.0.weight": head0_wgrad_reads_zeros}, "snd_head0.bwd")
    only_row_failing(P, {"gsact2": dgrad_masks_with_positive}, "snd3.dgrad")


def test_a_relu_mask_from_the_neighbouring_image_fails_its_own_row(stand_in):
    P, _ = stand_in

    def gact3_image1(v, b):                                        # image 1's gact3 under image 2's act3 gates
        v = v.clone()
        full = torch.nn.grad.conv2d_input(tuple(b["act3"].shape), P["imgBranch.6.weight"], b["gact4"], stride=2, padding=1)
        v[1] = full[1] * (b["act3"][2] > 0)
        return v

    def conv1_image3(v, b):                                        # conv 1's weight gradient with image 3 under image 4's act1 gates
        a = b["act1"].clone()
        a[3] = b["act1"][4]
        return kc.conv1_grads(b["gact2"], P["imgBranch.2.weight"], a, b["image"], v.shape)[0]

    def ghid_row0(v, b):                                           # the hidden gradient of image 0 under image 1's gates
        v = v.clone()
        v[0] = (b["graw_i"][0] @ P["imgTriplet.2.weight"]) * (b["hid_i"][1] > 0)
        return v

    only_row_failing(P, {"gact3": gact3_image1}, "conv4.dgrad")
    only_row_failing(P, {"G.imgBranch.0.weight": conv1_image3}, "conv1.grads")
    only_row_failing(P, {"ghid_i": ghid_row0}, "img_head2.bwd")


def test_a_nan_in_a_device_buffer_is_reported_as_inf(stand_in):
    """NaN compares false with everything: rel and ratio turn it into inf, so that no form of the pass condition lets it by."""
    P, b = stand_in
    for key, name in (("G.imgBranch.4.weight", "conv3.wgrad"), ("sact2", "snd2.fwd"), ("gact3", "conv4.dgrad"),
                      ("G.imgBranch.0.bias", "conv1.grads"), ("gsact4", "snd_head0.bwd"), ("G.soundTriplet.2.bias", "snd_head2.bgrad"), ("emb_i", "img_l2norm.fwd")):
        t = b[key].clone()
        t.view(-1)[t.numel() // 2] = float("nan")
        res = kc.check_layers(dict(b, **{key: t}), P, only=lambda n, name=name: n == name)
        q = worst(res, name)
        assert q == float("inf") and q > 1 and not q <= 1, (name, res)
    t = b["G.soundCNN.0.bias"].clone()
    t[3] = float("inf")
    image, snd, g_i, g_s = kc.make_inputs(STAND_IN)
    out, _, _ = kc.end_to_end(P, image, snd, g_i, g_s, dict(b, **{"G.soundCNN.0.bias": t}))
    assert kc.ratio(*out["arena"]) == float("inf") and kc.ratio(*out["G.soundCNN.0.bias"]) == float("inf")


def test_end_to_end_holds_the_devices_gates_and_sees_a_wrong_gradient(stand_in):
    P, b = stand_in
    image, snd, g_i, g_s = kc.make_inputs(STAND_IN)
    out, flips, units = kc.end_to_end(P, image, snd, g_i, g_s, b)
    assert units == 5 * (81312 + 2 * 2912)
    assert all(v <= tol for _k, _n, v, tol in flips) and sum(n for _k, n, _v, _t in flips) <= 1 + kc.FLIP_RATE * units, flips
    assert all(kc.ratio(e, d) <= 1 for e, d in out.values()), out
    wrong = dict(b)
    wrong["G.imgBranch.2.bias"] = b["G.imgBranch.2.bias"] + b["gact2"][4].sum((1, 2))
    out, _, _ = kc.end_to_end(P, image, snd, g_i, g_s, wrong)
    assert kc.ratio(*out["arena"]) > 1 and kc.ratio(*out["G.imgBranch.2.bias"]) > 1


@pytest.mark.parametrize("name", ["A", "B", "C", "D", "E"])
def test_the_gpu_cases_inputs_keep_the_fp32_stand_in_within_the_flip_cap(name):
    """The inputs themselves respect the end-to-end check's condition: with torch fp32 as the device, the ReLU gates that differ
    from float64's are near-ties and at most 1 + FLIP_RATE x gated units."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    case = kc.CASES[name]
    P = kc.seeded_params(case["seed"], case["h"])
    image, snd, g_i, g_s = kc.make_inputs(case)
    dev = kc.chain(P, image, snd, g_i, g_s)
    out, flips, units = kc.end_to_end(P, image, snd, g_i, g_s, dev)
    assert all(v <= tol for _k, _n, v, tol in flips), flips
    assert sum(n for _k, n, _v, _t in flips) <= 1 + kc.FLIP_RATE * units, (flips, units)
    assert all(kc.ratio(e, d) <= 1 for k, (e, d) in out.items() if not k.startswith("G.")), out


def test_the_emulated_bias_sum_is_the_same_sum_and_its_row_still_catches_a_missing_clip(stand_in):
    """kuka_layers_cpu.ORDER: snd_head2.bgrad is measured against the kernel's own order of additions.  The emulation is the
    column sum (at fp32 round-off, for every row count up to a few wave rounds), the unfaulted stand-in passes against it, and a
    bias gradient without one clip's row -- or with the last two rows, one step of one wave, dropped -- is far outside it."""
    P, b = stand_in
    assert set(kc.ORDER) == {"snd_head2.bgrad"}
    torch.manual_seed(4)
    for R in (1, 2, 3, 4, 5, 8, 9, 37, 74):
        g = torch.randn(R, 3)
        assert kc.rel(kc.bias_sum_seq(g), g.double().sum(0)) < 1e-6, R
    res = kc.check_layers(b, P, only=lambda n: n == "snd_head2.bgrad")
    assert worst(res, "snd_head2.bgrad") <= 1, res
    for rows in (slice(9, 10), slice(8, 10), slice(0, 1)):
        only_row_failing(P, {"G.soundTriplet.2.bias": lambda v, b, rows=rows: v - b["graw_s"][rows].sum(0)}, "snd_head2.bgrad")

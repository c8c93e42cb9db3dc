"""CPU-only checks of tests/ithor_layers_cpu.py, the float64 layer reference of tests/test_gpu_ithor_layers.py:
(1) chained in order, the layer functions reproduce oracle.torch_oracle.IthorNetCPU in float64 -- forward, torch.autograd backward
from dense cotangents, every intermediate map in the device's buffer layout -- to 1e-12; (2) with torch fp32 standing in for the
device, the single-layer checks pass the unfaulted result and catch one dropped border tap, 16 missing terms of one weight-gradient
element, one misrouted pool gradient and one GRU step fed its neighbour clip's state; (3) the emulation of the gather-GEMM's
accumulation order is the same product, faults in the layers measured against it are still caught, a NaN in any buffer is
reported, and the end-to-end check follows a gate that flipped at a near-tie without going blind."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.torch_oracle import ithor_seeded
from tests import ithor_layers_cpu as lc


def inputs(h, B, seed, u8=False):
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(B, 3, h, h), dtype=np.uint8)
    snd = (rng.standard_normal((2 * B, 1, 600, 40)) * 6.0).astype(np.float32)
    snd[0, :, 350:] = 0.0
    image = torch.from_numpy(img) if u8 else (torch.from_numpy(img) / 255.).float()
    g = torch.from_numpy(rng.standard_normal((3 * B, 3)))
    return image, torch.from_numpy(snd), g[:B], g[B:]


@pytest.mark.parametrize("h,B", [(84, 2), (96, 2)])
def test_chain_reproduces_the_oracle_in_float64(h, B):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    net = ithor_seeded(31).double()
    P = {k: v.detach() for k, v in net.named_parameters()}
    image, snd, g_i, g_s = inputs(h, B, 7 + h)
    got = lc.chain(P, image.double(), snd.double(), g_i, g_s)

    # the oracle, with every intermediate kept
    ref = {}

    def keep(name):
        def hook(_m, _i, out):
            out.retain_grad()
            ref[name] = out
        return hook

    hooks = [net.imgBranch[i].register_forward_hook(keep(n)) for i, n in
             ((1, "a1"), (3, "a2"), (4, "p2"), (6, "a3"), (7, "p3"), (9, "a4"), (10, "p4"), (12, "a5"), (13, "p5"), (16, "a6"))]
    hooks += [net.cnn[i].register_forward_hook(keep(n)) for i, n in ((1, "s1"), (3, "s2"), (5, "s3"))]
    hooks += [net.imgTriplet[1].register_forward_hook(keep("hid_i")), net.imgTriplet[2].register_forward_hook(keep("raw_i")),
              net.soundTriplet[1].register_forward_hook(keep("hid_s1")), net.soundTriplet[3].register_forward_hook(keep("hid_s2")),
              net.soundTriplet[4].register_forward_hook(keep("raw_s"))]
    seq = {}
    hooks.append(net.rnn.register_forward_hook(lambda _m, _i, out: seq.update(out=out[0])))
    x = image.double()
    emb_i = F.normalize(net.imgTriplet(net.imgBranch(x)), p=2, dim=1)
    sraw = net.sound_raw(snd.double())
    sraw.retain_grad()
    emb_s = F.normalize(net.soundTriplet(sraw), p=2, dim=1)
    torch.autograd.backward([emb_i, emb_s], [g_i, g_s])
    for hk in hooks:
        hk.remove()

    def close(name, a, r):
        assert a.shape == r.shape, (name, a.shape, r.shape)
        e = lc.rel(a, r.detach())
        assert e <= 1e-12, (name, e)

    close("emb_i", got["emb_i"], emb_i)
    close("emb_s", got["emb_s"], emb_s)
    close("sraw", got["sraw"], sraw)
    close("gsraw", got["gsraw"], sraw.grad)
    for k, r in ref.items():
        seqlay = k == "s3"
        close(k, got[k], lc.to_seq(r) if seqlay else r)
        gk = "g" + k if k[0] != "h" and k[0] != "r" else {"hid_i": "ghid_i", "hid_s1": "ghid_s1", "hid_s2": "ghid_s2",
                                                          "raw_i": "graw_i", "raw_s": "graw_s"}[k]
        # the device keeps gradients wrt PRE-activations: autograd's gradient wrt a ReLU's output, times that ReLU's gate
        # (pooled maps and the un-normalised embeddings have no gate)
        gr = r.grad if k[0] in "pr" else r.grad * (r > 0)
        close(gk, got[gk], lc.to_seq(gr) if seqlay else gr)
    out = seq["out"]                                             # (clips, 73, 1024): [forward h_t | reverse h_t]
    for s in range(lc.T):
        close(f"hb0[{s + 1}]", got["hb"][0, s + 1], out[:, s, :lc.GH])
        close(f"hb1[{s + 1}]", got["hb"][1, s + 1], out[:, lc.T - 1 - s, lc.GH:])
    assert float(got["hb"][:, 0].abs().max()) == 0
    for k, p in net.named_parameters():
        close("G." + k, got["G." + k], p.grad)
    # and every single-layer check holds on the chain's own buffers at float64 round-off
    for name, _kind, fn, ins, outs in lc.layer_table(got, P):
        for o, r in zip(outs, lc._tuple(fn(*ins))):
            assert lc.rel(o, r) <= 1e-12, name


@pytest.fixture(scope="module")
def stand_in():
    """torch fp32 as the device: every buffer of a forward and backward at h = 84, B = 2 from the fp32 chain."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    net = ithor_seeded(31)
    P = {k: v.detach() for k, v in net.named_parameters()}
    image, snd, g_i, g_s = inputs(84, 2, 91, u8=True)
    return P, lc.chain(P, image, snd, g_i, g_s)


def worst(res, name):
    return max(q for _e, _d, q in res[name][1])


def test_unfaulted_fp32_stand_in_passes_every_layer(stand_in):
    P, b = stand_in
    res = lc.check_layers(b, P)
    assert len(res) >= 50
    kinds = {k for k, _ in res.values()}
    assert {"conv fwd", "conv dgrad", "conv wgrad", "conv bgrad", "pool fwd", "pool+relu bwd", "linear fwd", "linear bwd",
            "gru step fwd", "gru gates bwd", "gru wgrad", "gru dgrad", "gru concat", "l2norm fwd", "l2norm bwd"} <= kinds
    for name in res:
        assert worst(res, name) <= 1, (name, res[name])


def faulted(b, **changed):
    c = dict(b)
    c.update(changed)
    return c


def test_a_dropped_border_tap_is_caught(stand_in):
    P, b = stand_in
    # conv 3 (64 x 42 x 42 from p2): output row 0 of one channel of one image misses the tap (ky, kx) = (2, 0)
    w = P["imgBranch.5.weight"].clone()
    w[:, :, 2, 0] = 0
    a3 = b["a3"].clone()
    a3[1, 5, 0] = lc.conv_fwd(b["p2"], w, P["imgBranch.5.bias"], "i")[1, 5, 0]
    res = lc.check_layers(faulted(b, a3=a3), P, only=lambda n: n == "conv3.fwd")
    assert worst(res, "conv3.fwd") > 1, res
    # the same on the first sound convolution's last output row
    w = P["cnn.0.weight"].clone()
    w[:, :, 0, 10] = 0
    s1 = b["s1"].clone()
    s1[3, 7, 299] = lc.conv_fwd(b["snd"], w, P["cnn.0.bias"], "s1")[3, 7, 299]
    res = lc.check_layers(faulted(b, s1=s1), P, only=lambda n: n == "snd1.fwd")
    assert worst(res, "snd1.fwd") > 1, res


def test_sixteen_missing_terms_of_one_weight_gradient_element_are_caught(stand_in):
    P, b = stand_in
    # k runs over (image, oy, ox): the last 16 are the end of the last image's last row
    # (of the first output and input channels that are alive there; many maps of the seeded model are dead past a ReLU)
    for name, x, g, key, ky, kx in (("conv3.wgrad", b["p2"], b["ga3"], "G.imgBranch.5.weight", 1, 1),
                                    ("snd2.wgrad", b["s1"], b["gs2"], "G.cnn.2.weight", 5, 2)):
        co = int(torch.nonzero(g[-1].flatten(1)[:, -16:].abs().sum(1))[0])
        ci = int(torch.nonzero(x[-1, :, -3:].abs().sum((1, 2)))[0])
        el = (co, ci, ky, kx)
        st, (ph, pw) = lc.GEO["i" if name[0] == "c" else "s2"]
        miss, W = 0.0, g.shape[-1]
        for q in range(g.shape[-2] * W - 16, g.shape[-2] * W):
            oy, ox = divmod(q, W)
            iy, ix = oy * st - ph + ky, ox * st - pw + kx
            if 0 <= iy < x.shape[-2] and 0 <= ix < x.shape[-1]:
                miss += float(g[-1, co, oy, ox]) * float(x[-1, ci, iy, ix])
        assert miss != 0.0
        G = b[key].clone()
        G[el] -= miss
        res = lc.check_layers(faulted(b, **{key: G}), P, only=lambda n, name=name: n == name)
        assert worst(res, name) > 1, (name, miss, res)


def test_a_misrouted_pool_gradient_is_caught(stand_in):
    P, b = stand_in
    for l in (2, 4):                                             # even map (42 <- 84) and odd map (21 -> 10)
        ga = b[f"ga{l}"].clone()
        nz = torch.nonzero(ga)                                   # (many maps of the seeded model are dead: take a live cell)
        i, c, y, x = (int(v) for v in nz[len(nz) // 2])
        x2 = x ^ 1                                               # the neighbouring cell of the same window
        ga[i, c, y, x2], ga[i, c, y, x] = ga[i, c, y, x].item(), 0.0
        res = lc.check_layers(faulted(b, **{f"ga{l}": ga}), P, only=lambda n, l=l: n == f"pool{l}.bwd")
        assert worst(res, f"pool{l}.bwd") > 1, res


def test_pool_ties_counts_positive_repeated_maxima():
    a = torch.tensor([[[[1., 1., 0., 0., 5.], [0., 0., 0., 0., 5.], [2., 3., -1., -1., 5.], [3., 1., -1., -1., 5.], [7., 7., 7., 7., 7.]]]])
    assert lc.pool_ties(a) == 2                                  # (1, 1 | .) and (. 3 | 3 .); zero and negative ties and the odd edge do not count


def test_a_gru_step_fed_the_neighbour_clips_state_is_caught(stand_in):
    P, b = stand_in
    _w_ih, w_hh, _b_ih, b_hh = lc.rnn_params(P)
    for d, s in ((0, 40), (1, 72)):
        hb_in = b["hb"].clone()
        hb_in[d, s, 1] = b["hb"][d, s, 0]                        # clip 1 reads clip 0's h[t-1] at this one step
        wrong = lc.gru_fwd(hb_in, b["gi"], w_hh, b_hh)[d, s, 1]
        hb = b["hb"].clone()
        hb[d, s + 1, 1] = wrong
        res = lc.check_layers(faulted(b, hb=hb), P, only=lambda n: n == "gru.fwd")
        assert worst(res, "gru.fwd") > 1, (d, s, res)


def test_layer_distance_is_the_fp32_cpu_distance():
    torch.manual_seed(3)
    x, w, c = torch.randn(5, 33), torch.randn(7, 33), torch.randn(7)
    d = lc.layer_distance(lambda x, w, c: lc.linear_fwd(x, w, c, False), [x, w, c])
    ref = x.double() @ w.double().t() + c.double()
    assert d == float(((x @ w.t() + c).double() - ref).abs().max() / ref.abs().max())
    assert 0 < d < 1e-6
    assert lc.layer_distance(lc.pool_fwd, [torch.randn(1, 2, 5, 5)]) == 0.0          # routing is exact
    assert lc.ratio(0.0, 0.0) == 0.0 and lc.ratio(1e-9, 0.0) == float("inf") and lc.ratio(4e-7, 1e-7) == 1.0


def test_accumulation_order_emulation_is_the_same_product():
    """seq_dot / conv_fwd_seq (the gather-GEMM's one-accumulator order) compute the layer itself, at fp32 round-off."""
    torch.manual_seed(5)
    x, w, c = torch.randn(3, 4, 9, 8), torch.randn(6, 4, 11, 5) / 15, torch.randn(6)
    ref = lc.conv_fwd(x.double(), w.double(), c.double(), "s2")
    assert lc.rel(lc.conv_fwd_seq(x, w, c, "s2", [0, 2]), ref[[0, 2]]) < 2e-6
    a, v, d = torch.randn(7, 33), torch.randn(5, 33), torch.randn(5)
    assert lc.rel(lc.linear_fwd_seq(a, v, d, True), lc.linear_fwd(a.double(), v.double(), d.double(), True)) < 1e-6
    assert set(lc.ORDER) == {"snd2.fwd", "conv6.fwd", "img_head0.fwd", "snd_head0.fwd"}


def test_end_to_end_holds_the_devices_gates(stand_in):
    """The end-to-end check follows a gate that flipped at a near-tie, reports it, and still sees a wrong gradient."""
    P, b = stand_in
    image, snd, g_i, g_s = inputs(84, 2, 91, u8=True)
    out, flips, units = lc.end_to_end(P, image, snd, g_i, g_s, b)
    assert units > 3e6 and all(v <= tol for _k, _n, v, tol in flips) and sum(n for _k, n, _v, _t in flips) <= 1 + lc.FLIP_RATE * units
    assert all(lc.ratio(e, d) <= 1 for e, d in out.values()), out
    # a unit of a2 that float64 has off, in a window of zeros, comes out as 1e-9 on the "device": its window's gradient passes
    a2 = b["a2"].clone()
    dead = torch.nonzero((lc.pool_fwd(b["a2"]) == 0) & (b["gp2"] != 0))
    i, c, y, x = (int(v) for v in dead[len(dead) // 2])
    a2[i, c, 2 * y + 1, 2 * x] = 1e-9
    fwd = {k: (a2 if k == "a2" else v) for k, v in b.items() if k in lc.FORWARD}
    dev = lc.chain(P, image, snd, g_i, g_s, gates={k: fwd[k] for k in lc.GATED}, forward=fwd)
    assert not torch.equal(dev["G.imgBranch.2.bias"], b["G.imgBranch.2.bias"])
    out, flips, _ = lc.end_to_end(P, image, snd, g_i, g_s, dev)
    assert [(k, n) for k, n, _v, _t in flips] == [("a2", 1)] and flips[0][2] <= flips[0][3]
    assert all(lc.ratio(e, d) <= 1 for e, d in out.values()), out
    # the same flip at a value no rounding explains is reported beyond its allowance
    fwd["a2"] = a2.clone()
    fwd["a2"][i, c, 2 * y + 1, 2 * x] = 1e-3
    _, flips, _ = lc.end_to_end(P, image, snd, g_i, g_s, dict(dev, a2=fwd["a2"]))
    assert flips[0][2] > flips[0][3]
    # and a gradient that is wrong at the device's gates is still caught
    wrong = dict(dev)
    wrong["G.imgBranch.2.bias"] = dev["G.imgBranch.2.bias"] + b["gp2"][i, c, y, x]
    out, _, _ = lc.end_to_end(P, image, snd, g_i, g_s, wrong)
    assert lc.ratio(*out["arena"]) > 1 and lc.ratio(*out["G.imgBranch.2.bias"]) > 1


def test_faults_in_the_layers_with_the_emulated_yardstick_are_caught(stand_in):
    """The four layers of ORDER have the looser yardstick (the kernel's one-accumulator order): a dropped tap in one output row
    and a dropped last chunk of 16 k in one output are still far outside it."""
    P, b = stand_in
    res = lc.check_layers(b, P, only=lambda n: n in lc.ORDER)
    assert set(res) == set(lc.ORDER) and all(worst(res, n) <= 1 for n in res), res
    # sound conv 2: the last output row of one channel of the LAST clip misses the tap (ky, kx) = (0, 4)
    w = P["cnn.2.weight"].clone()
    w[:, :, 0, 4] = 0
    s2 = b["s2"].clone()
    s2[3, 9, 149] = lc.conv_fwd(b["s1"], w, P["cnn.2.bias"], "s2")[3, 9, 149]
    assert not torch.equal(s2, b["s2"])
    res = lc.check_layers(faulted(b, s2=s2), P, only=lambda n: n == "snd2.fwd")
    assert worst(res, "snd2.fwd") > 1, res
    # conv 6 and the two heads' first layers: one output misses one chunk of 16 k (conv 6: k = (ci, ky, kx); output pixel (1, 1)
    # of the stride-2, pad-1 convolution reads rows / columns 1..3).  Many units of the seeded model are dead past a ReLU, so it
    # is the last chunk in which some input is alive, and the first output that is alive and whose missing terms are not zero.
    def last_live_chunk(x):
        c = int(torch.nonzero(x.reshape(x.shape[0], -1, 16).abs().sum((0, 2)))[-1])
        return slice(16 * c, 16 * c + 16)

    def first_live(y, miss):
        hit = torch.nonzero((miss != 0) & (y > miss.abs()))
        assert len(hit), "no live output with live missing terms"
        return tuple(int(v) for v in hit[0])

    patch = b["p5"][:, :, 1:4, 1:4].flatten(1)                   # (B, 1152)
    ks = last_live_chunk(patch)
    miss = patch[:, ks] @ P["imgBranch.14.weight"].flatten(1)[:, ks].t()              # (B, 128)
    a6 = b["a6"].clone().view(-1, 128, 3, 3)
    i, c = first_live(a6[:, :, 1, 1], miss)
    a6[i, c, 1, 1] -= miss[i, c]
    res = lc.check_layers(faulted(b, a6=a6.view(-1, 1152)), P, only=lambda n: n == "conv6.fwd")
    assert worst(res, "conv6.fwd") > 1, (float(miss[i, c]), res)
    for name, xk, lin, yk in (("img_head0.fwd", "a6", "imgTriplet.0", "hid_i"), ("snd_head0.fwd", "sraw", "soundTriplet.0", "hid_s1")):
        ks = last_live_chunk(b[xk])
        miss = b[xk][:, ks] @ P[lin + ".weight"][:, ks].t()
        y = b[yk].clone()
        row, o = first_live(y, miss)
        y[row, o] -= miss[row, o]
        res = lc.check_layers(faulted(b, **{yk: y}), P, only=lambda n, name=name: n == name)
        assert worst(res, name) > 1, (name, float(miss[row, o]), res)


def test_a_nan_in_a_device_buffer_is_reported(stand_in):
    """NaN compares false with everything: rel and ratio turn it into inf, so that no form of the pass condition lets it by."""
    P, b = stand_in
    for key, name in (("G.imgBranch.5.weight", "conv3.wgrad"), ("s2", "snd2.fwd"), ("ga4", "pool4.bwd"), ("dgh", "gru.bwd")):
        t = b[key].clone()
        t.view(-1)[t.numel() // 2] = float("nan")
        res = lc.check_layers(faulted(b, **{key: t}), P, only=lambda n, name=name: n == name)
        q = worst(res, name)
        assert q == float("inf") and q > 1 and not q <= 1, (name, res)
    t = b["G.cnn.0.bias"].clone()
    t[3] = float("inf")
    image, snd, g_i, g_s = inputs(84, 2, 91, u8=True)
    out, _, _ = lc.end_to_end(P, image, snd, g_i, g_s, faulted(b, **{"G.cnn.0.bias": t}))
    assert lc.ratio(*out["arena"]) == float("inf") and lc.ratio(*out["G.cnn.0.bias"]) == float("inf")
    assert lc.ratio(float("nan"), 1e-7) == float("inf") and lc.ratio(1e-7, float("nan")) == float("inf")
    assert lc.rel(torch.tensor([1.0, float("nan")]), torch.tensor([1.0, 2.0])) == float("inf")

"""GPU checks of the convolution stacks' bf16 mode (csrc/convstack.hip: var_convstack_fwd_ex / var_convstack_bwd_ex with flags
bit 0; var_amd.conv_stack_eval(precision="bf16") / bind_convs(policy, precision="bf16")) against the layer-by-layer float64
restatement of tests/convstack_bf16_cpu.py.

Every numeric check is LOCAL TO ONE LAYER: a layer's forward map, weight gradient, bias gradient and gated data gradient are
recomputed in float64 on bf16-rounded operands from the buffers the GPU itself returned below (or above) that layer -- `saved`,
`grad_maps`, the parameters, the image -- so a ReLU gate that falls the other way cannot carry into another comparison.  Bounds are
measured, not chosen (convstack_bf16_cpu.bounds): per array four times the distance of torch's own fp32 CPU evaluation of the same
rounded-operand product from its float64 evaluation, the largest over the draws (20 up to B = 5, 3 beyond), relative to the
array's largest magnitude.  Every test prints what it measured before it asserts.

Which kernels serve a layer is the library's business (the gather-GEMM with rounded operands, or img_bf16.hip's kernels); the
grid-wrap sizes below come from img_bf16.hip's launch code: a persistent kernel with T tiles per image and a grid cap of G
workgroups wraps at B = floor(G / T) | + 1."""
import ctypes

import numpy as np
import pytest
import torch

from tests import convstack_bf16_cpu as cb
from tests import convstack_cpu as cc
from tests import trunk_cpu as tc

pytestmark = pytest.mark.gpu
SENT = -77.0


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


@pytest.fixture(scope="module")
def ctx(var_amd):
    from var_amd._lib import Context
    return Context.get(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def run(var_amd, kind, P, d, precision="bf16", maps=True, module=None, on_device=False):
    """conv_stack_eval forward + backward: 'feat', 'act.<l>', 'g.<l>' (with maps), 'd.<parameter>' as numpy arrays (on_device:
    CUDA tensors, for the large batches)."""
    module = cc.stack_module(kind, P).cuda() if module is None else module
    image = dev(d["image"])
    n_saved = var_amd.load_library().var_convstack_saved_floats(kind, image.shape[0])
    gm = torch.full((n_saved,), SENT, device="cuda") if maps else None
    feat, saved, smap = var_amd.conv_stack_eval(module, image, return_saved=True, precision=precision, grad_maps=gm)
    params = dict(module.named_parameters())
    grads = torch.autograd.grad((feat * dev(d["d_feat"])).sum(), [params[k] for k in cc.param_names(kind)])
    out = (lambda t: t.detach()) if on_device else host
    res = {"feat": out(feat)}
    sv, gv = out(saved), (out(gm) if maps else None)
    for name, (off, shape) in smap.items():
        n = int(np.prod(shape))
        res["act." + name] = sv[off:off + n].reshape(shape)
        if maps:
            res["g." + name] = gv[off:off + n].reshape(shape)
    res.update({"d." + k: out(g) for k, g in zip(cc.param_names(kind), grads)})
    assert np.array_equal(host(image), d["image"])
    return res


def parity(kind, P, d, got, bound, label):
    """Every layer of `got` against its float64 reference on the GPU's own buffers; returns the worst error / bound."""
    ref = cb.layer_refs(kind, P, d, got)
    last = cc.layer_names(kind)[-1]
    assert cb.nontrivial(kind, got), "a map without positive or without zero units, or a zero gradient array"
    assert set(ref) == set(bound)
    worst = (0.0, None)
    for k in sorted(ref):
        if k == "g." + last:                                          # a selection of d_feat: exact
            assert np.array_equal(got[k].astype(np.float64), ref[k]), k
            continue
        err = cb.rel(got[k], ref[k])
        assert bound[k] > 0 and np.abs(ref[k]).max() > 0, k
        print(f"    {label} {k}: error {err:.3g}, bound {bound[k]:.3g}, fraction {err / bound[k]:.3f}")
        worst = max(worst, (err / bound[k], (k, err, bound[k])))
    return worst


# ---- 1: layer parity ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,u8", cb.PARITY_CASES)
def test_every_layer_matches_float64_on_rounded_operands(var_amd, kind, B, u8):
    P, d = cc.convstack_params(kind, cb.PARITY_SEED), cc.convstack_data(kind, B, cb.PARITY_SEED, u8=u8)
    got = run(var_amd, kind, P, d)
    assert np.array_equal(bits(got["feat"]), bits(got["act." + cc.layer_names(kind)[-1]].reshape(B, -1)))
    worst = parity(kind, P, d, got, cb.bounds(kind, B), f"kind {kind} B {B} {'u8' if u8 else 'f32'}")
    print(f"kind {kind} B {B} {'u8' if u8 else 'f32'}: worst error / bound {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0, worst


@pytest.mark.parametrize("kind", [0, 1])
def test_an_image_of_all_byte_values_and_its_float_twin(var_amd, kind):
    P, d = cb.all_bytes_case(kind)
    module = cc.stack_module(kind, P).cuda()
    got = run(var_amd, kind, P, d, module=module)
    worst = parity(kind, P, d, got, cb.bounds(kind, 1), f"kind {kind} all bytes")
    print(f"kind {kind} all 256 byte values: worst error / bound {worst[0]:.3f} at {worst[1]}")
    twin = run(var_amd, kind, P, dict(d, image=cc.as_float_image(d["image"])), module=module)
    assert set(twin) == set(got)
    for k in got:
        assert np.array_equal(bits(got[k]), bits(twin[k])), k
    assert worst[0] <= 1.0, worst


# ---- 2: more tiles than the grid ----------------------------------------------------------------------------------------------------
# (kind, B, forward / data-gradient layers whose persistent kernel wraps between B - 1 and B, weight-gradient layers likewise)
# img_bf16.hip: c3_kernel has side / TR tiles per image (NI images per tile at 12 x 12) and at most 256 * WGS workgroups, c3w_kernel
# side / 4 tiles per image and at most 512.  Kind 1: 32->32 at 96 (TR 8, cap 512: 42 | 43; c3w 21 | 22), 32->64 at 48 (TR 8: 85 | 86;
# c3w 42 | 43), 64->64 at 24 (whole images, cap 256: 256 | 257), 64->128 at 12 (two images, cap 256: 512 | 513).  Kind 0 adds
# 64->64 at 48 (forward TR 8: 85 | 86; data gradient TR 4: 42 | 43; c3w 42 | 43), 64->128 at 24 (TR 12, cap 256: 128 | 129) and
# 128->128 at 24 (forward TR 12: 128 | 129; data gradient TR 8: 85 | 86).
# Layer names: kind 1 "2" 32->32 at 96, "5" 32->64 at 48, "8" 64->64 at 24, "11" 64->128 at 12; kind 0 "7" 64->64 at 48, "10" 64->128
# at 24, "12" 128->128 at 24 (its "2" and "5" are kind 1's kernels).
WRAPS = [(1, 22, (), ("2",)), (1, 43, ("2",), ("5",)), (1, 86, ("5",), ()), (1, 257, ("8",), ()), (1, 513, ("11",), ()),
         (0, 43, ("7",), ("7",)), (0, 86, ("7", "12"), ()), (0, 129, ("10", "12"), ())]


@pytest.mark.parametrize("kind,B,conv_layers,wgrad_layers", WRAPS)
def test_more_tiles_than_the_grid(var_amd, kind, B, conv_layers, wgrad_layers):
    seed = 90 + B
    P, d = cc.convstack_params(kind, seed), cc.convstack_data(kind, B, seed)
    got = run(var_amd, kind, P, d, on_device=True)
    names = list(cc.layer_names(kind))
    # forward and data gradient are per image: the first two images and the two on either side of the wrap (image B - 1 is the
    # first whose tiles lie beyond the grid).  The bound is that of a batch of as many images: the products are per image, and the
    # distance is relative to the largest magnitude of the compared array
    images = [0, 1, B - 2, B - 1]
    sub = {"image": d["image"][images], "d_feat": d["d_feat"][images]}
    small = {k: host(v[images]) for k, v in got.items() if k.startswith(("act.", "g."))}
    bound = cb.bounds(kind, len(images)) if conv_layers else {}
    worst = (0.0, None)
    for n in conv_layers:
        l = names.index(n)
        below = names[l - 1]
        # forward of layer n from the GPU's map below; the gated data gradient g_below from the GPU's g_n
        ref = cb.layer_refs(kind, P, sub, small, what=("act",), layers=[n])
        ref.update(cb.layer_refs(kind, P, sub, small, what=("g",), layers=[below]))
        for k in sorted(ref):
            err = cb.rel(small[k], ref[k])
            assert np.abs(ref[k]).max() > 0, k
            print(f"    kind {kind} B {B} images {images} {k}: error {err:.3g}, bound {bound[k]:.3g}, fraction {err / bound[k]:.3f}")
            worst = max(worst, (err / bound[k], (k, err, bound[k])))
    for n in wgrad_layers:                                            # weight gradients whole, for the layer concerned
        l = names.index(n)
        geo = cb.geometry(kind)[l]
        x = got["act." + names[l - 1]].cpu()
        x = cb.pool(x) if cb.geometry(kind)[l - 1][5] else x
        g = got["g." + n].cpu()
        ref = cb.weight_grad(x, g, P[n + ".weight"].shape, geo[3], geo[4], torch.float64).numpy()
        err, b = cb.rel(host(got["d." + n + ".weight"]), ref), cb.weight_grad_bound(kind, B, n)
        print(f"    kind {kind} B {B} d.{n}.weight: error {err:.3g}, bound {b:.3g}, fraction {err / b:.3f}")
        worst = max(worst, (err / b, ("d." + n + ".weight", err, b)))
    print(f"kind {kind} B {B}: worst error / bound {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0, worst


# ---- 3: bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_two_runs_give_equal_bits(var_amd, kind):
    B = 6
    P, d = cc.convstack_params(kind, 31), cc.convstack_data(kind, B, 31)
    module = cc.stack_module(kind, P).cuda()
    a, b = run(var_amd, kind, P, d, module=module), run(var_amd, kind, P, d, module=module)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    # the mode is not the fp32 path under another name
    c = run(var_amd, kind, P, d, precision="fp32", module=module)
    assert not np.array_equal(bits(a["feat"]), bits(c["feat"]))
    assert cb.rel(a["feat"], c["feat"]) < 0.05


@pytest.mark.parametrize("kind", [0, 1])
def test_forward_and_backward_replay_from_a_captured_graph(var_amd, kind):
    from var_amd._lib import new_graph
    B = 3
    P = cc.convstack_params(kind, 40)
    draws = [cc.convstack_data(kind, B, 40 + i) for i in range(3)]
    module = cc.stack_module(kind, P).cuda()
    eager = [run(var_amd, kind, P, d, maps=False, module=module) for d in draws]
    static = {k: dev(draws[0][k]) for k in ("image", "d_feat")}
    params = dict(module.named_parameters())
    leaves = [params[k] for k in cc.param_names(kind)]
    g = new_graph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        feat = var_amd.conv_stack_eval(module, static["image"], precision="bf16")
        grads = torch.autograd.grad((feat * static["d_feat"]).sum(), leaves)
    torch.cuda.current_stream().wait_stream(side)
    for i in (1, 2):
        with torch.no_grad():
            for k in static:
                static[k].copy_(dev(draws[i][k]))
        g.replay()
        got = {"feat": host(feat)}
        got.update({"d." + k: host(v) for k, v in zip(cc.param_names(kind), grads)})
        for k in got:
            assert np.array_equal(bits(got[k]), bits(eager[i][k])), (i, k)


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Call:
    """Buffers of one var_convstack_fwd_ex + var_convstack_bwd_ex pair, every output inside a sentinel-filled buffer with PAD floats
    on each side."""
    PAD = 64

    def __init__(self, lib, kind, B, flags, seed=3, u8=True):
        self.lib, self.kind, self.B, self.u8, self.flags = lib, kind, B, u8, flags
        self.P, self.d = cc.convstack_params(kind, seed), cc.convstack_data(kind, B, seed, u8=u8)
        self.params = [dev(self.P[k]) for k in cc.param_names(kind)]
        self.table = (ctypes.c_void_p * len(self.params))(*(t.data_ptr() for t in self.params))
        self.inp = {k: dev(self.d[k]) for k in ("image", "d_feat")}
        self.n_saved = lib.var_convstack_saved_floats(kind, B)
        self.n_grad = lib.var_convstack_grad_offset(kind, len(self.params))
        self.ws_bytes = lib.var_convstack_workspace_bytes_ex(kind, B, flags)
        self.size = {"feat": B * cc.feat_width(kind), "saved": self.n_saved, "grads": self.n_grad, "gmaps": self.n_saved,
                     "ws": self.ws_bytes // 4}
        self.buf = {k: torch.full((n + 2 * self.PAD,), SENT, device="cuda") for k, n in self.size.items()}
        self.out = {k: b[self.PAD:self.PAD + self.size[k]] for k, b in self.buf.items()}
        self.bstride = int(np.prod(cc.STACKS[kind][0]))

    def _common(self, over):
        a = dict(kind=self.kind, params=self.table, image=p(self.inp["image"]), u8=int(self.u8), bstride=self.bstride, B=self.B,
                 feat=p(self.out["feat"]), saved=p(self.out["saved"]), d_feat=p(self.inp["d_feat"]), grads=p(self.out["grads"]),
                 ws=p(self.out["ws"]), ws_bytes=self.ws_bytes, gmaps=p(self.out["gmaps"]), flags=self.flags)
        a.update(over)
        return a

    def fwd(self, **over):
        from var_amd._lib import Context
        a = self._common(over)
        return self.lib.var_convstack_fwd_ex(Context.get(0).handle, None, a["kind"], a["params"], a["image"], a["u8"], a["bstride"],
                                             a["B"], a["feat"], a["saved"], a["ws"], a["ws_bytes"], a["flags"])

    def bwd(self, **over):
        from var_amd._lib import Context
        a = self._common(over)
        return self.lib.var_convstack_bwd_ex(Context.get(0).handle, None, a["kind"], a["params"], a["image"], a["u8"], a["bstride"],
                                             a["B"], a["saved"], a["d_feat"], a["grads"], a["ws"], a["ws_bytes"], a["gmaps"], a["flags"])

    def old_pair(self):
        """The entries without _ex into fresh buffers: (feat, saved, grads)."""
        from var_amd._lib import Context
        h = Context.get(0).handle
        feat, saved, grads = (torch.full((self.size[k],), SENT, device="cuda") for k in ("feat", "saved", "grads"))
        nb = self.lib.var_convstack_workspace_bytes(self.kind, self.B)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        assert self.lib.var_convstack_fwd(h, None, self.kind, self.table, p(self.inp["image"]), int(self.u8), self.bstride, self.B, p(feat),
                                          p(saved), p(ws), nb) == 0
        assert self.lib.var_convstack_bwd(h, None, self.kind, self.table, p(self.inp["image"]), int(self.u8), self.bstride, self.B, p(saved),
                                          p(self.inp["d_feat"]), p(grads), p(ws), nb) == 0
        return feat, saved, grads

    def pads_intact(self):
        torch.cuda.synchronize()
        return all(bool((b[:self.PAD] == SENT).all()) and bool((b[self.PAD + self.size[k]:] == SENT).all()) for k, b in self.buf.items())

    def untouched(self, names):
        torch.cuda.synchronize()
        return all(bool((self.buf[k] == SENT).all()) for k in names)


@pytest.mark.parametrize("kind,flags", [(0, 1), (1, 1), (2, 1), (0, 0), (1, 0), (2, 0)])
def test_outputs_are_fully_overwritten_and_nothing_outside_them(var_amd, ctx, kind, flags):
    B = 5
    c = Call(ctx.lib, kind, B, flags)
    assert c.fwd() == 0, ctx.lib.var_last_error(ctx.handle)
    assert c.pads_intact() and c.untouched(("grads", "gmaps"))
    assert not bool((c.out["feat"] == SENT).any()) and not bool((c.out["saved"] == SENT).any())
    before = {k: c.out[k].clone() for k in ("feat", "saved")}
    assert c.bwd() == 0, ctx.lib.var_last_error(ctx.handle)
    assert c.pads_intact()
    for k in before:
        assert torch.equal(before[k], c.out[k]), k
    assert not bool((c.out["grads"] == SENT).any()) and not bool((c.out["gmaps"] == SENT).any())
    assert np.array_equal(host(c.inp["image"]), c.d["image"]) and np.array_equal(host(c.inp["d_feat"]), c.d["d_feat"])
    for t, k in zip(c.params, cc.param_names(kind)):
        assert np.array_equal(host(t), c.P[k]), k
    # without d_saved: the same gradients, bit for bit, and the maps' buffer untouched
    c2 = Call(ctx.lib, kind, B, flags)
    assert c2.fwd() == 0 and c2.bwd(gmaps=None) == 0
    assert c2.pads_intact() and c2.untouched(("gmaps",))
    assert torch.equal(c2.out["grads"], c.out["grads"]) and torch.equal(c2.out["feat"], c.out["feat"])
    # the numbers are conv_stack_eval's
    got = run(var_amd, kind, c.P, c.d, precision="bf16" if flags else "fp32")
    assert np.array_equal(bits(host(c.out["feat"])), bits(got["feat"].ravel()))
    assert np.array_equal(bits(host(c.out["grads"])), bits(np.concatenate([got["d." + k].ravel() for k in cc.param_names(kind)])))
    assert np.array_equal(bits(host(c.out["gmaps"])), bits(np.concatenate([got["g." + n].ravel() for n in cc.layer_names(kind)])))
    old = c.old_pair()
    same = [torch.equal(a, b) for a, b in zip(old, (c.out["feat"], c.out["saved"], c.out["grads"]))]
    if flags == 0 or kind == 2:                                       # fp32 through _ex, and kind 2 under the flag: the old entries' bits
        assert all(same), same
    else:
        assert not any(same), same


def test_refused_calls_launch_nothing(ctx):
    lib = ctx.lib
    for kind in (0, 1, 2):
        c = Call(lib, kind, 2, 1)
        odd = ctypes.c_void_p(c.out["gmaps"].data_ptr() + 4)
        small = lib.var_convstack_workspace_bytes_ex(kind, 2, 0)
        bad = [dict(flags=2), dict(flags=3), dict(flags=-2), dict(flags=1 << 8)]
        if small != c.ws_bytes:
            bad.append(dict(ws_bytes=small))
        for over in bad + [dict(ws_bytes=c.ws_bytes - 1)]:
            assert c.fwd(**over) == -1, ("fwd", kind, over)
            assert lib.var_last_error(ctx.handle).decode().startswith("var_convstack_fwd_ex"), over
        for over in bad + [dict(ws_bytes=c.ws_bytes - 1), dict(gmaps=odd)]:
            assert c.bwd(**over) == -1, ("bwd", kind, over)
            assert lib.var_last_error(ctx.handle).decode().startswith("var_convstack_bwd_ex"), over
        assert c.untouched(("feat", "saved", "grads", "gmaps", "ws"))
        assert c.fwd() == 0 and c.bwd() == 0                          # and a good pair right after the refused ones
        assert c.pads_intact() and not bool((c.out["grads"] == SENT).any())
    module = cc.stack_module(0, cc.convstack_params(0, 1)).cuda()
    import var_amd
    image = torch.zeros(2, 3, 96, 96, dtype=torch.uint8, device="cuda")
    n = lib.var_convstack_saved_floats(0, 2)
    for gm in (torch.zeros(n - 4, device="cuda"), torch.zeros(n, device="cuda", dtype=torch.float64), torch.zeros(n)):
        with pytest.raises(var_amd.VarHipError):
            var_amd.conv_stack_eval(module, image, precision="bf16", grad_maps=gm)


# ---- 4: the binding --------------------------------------------------------------------------------------------------------------------
T, N = 3, 2


def real_policy(kind, Q):
    pol = tc.drop_in_policy(kind, 0).to("cuda")
    assert set(dict(pol.named_parameters())) == set(Q)
    with torch.no_grad():
        for k, v in pol.named_parameters():
            v.copy_(dev(Q[k]))
    assert pol._arena_intact()
    return pol


def sample_tuple(kind, s):
    obs = {k: dev(s[k]) for k in ("image", "image_feat", "goal_sound_feat") + (("occupancy",) if kind else ("robot_pose",))}
    return (obs,) + tuple(dev(s[k]) for k in ("hxs", "actions", "value_preds", "returns", "masks", "old_logp", "adv"))


@pytest.mark.parametrize("kind,n_act", [(0, 2), (1, 8)])
def test_ppo_loss_through_bf16_bind_convs_fills_every_gradient(var_amd, kind, n_act, monkeypatch):
    from var_amd import convstack as vc
    Q = cc.policy_params(kind, 9, n_act)
    s = cc.ppo_sample(kind, Q, T, N, n_act, 509)
    pol = real_policy(kind, Q)
    assert var_amd.bind_convs(pol, precision="bf16") is pol
    agent = var_amd.PPO(pol, tc.CLIP, 1, 1, tc.VCOEF, tc.ECOEF, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    # what the bound forward's image stack saved, and the d_feat the loss sends into it: the binding's own call, with the saved maps
    # and the gradient maps asked for
    seen, inner = {}, vc.conv_stack_eval

    def spy(module, image, return_saved=False, precision="fp32", grad_maps=None):
        if module is not pol.base.imgCNN:
            return inner(module, image, return_saved, precision, grad_maps)
        seen["precision"] = precision
        seen["gm"] = torch.full((var_amd.load_library().var_convstack_saved_floats(kind, image.shape[0]),), SENT, device="cuda")
        feat, seen["saved"], seen["smap"] = inner(module, image, True, precision, seen["gm"])
        feat.register_hook(lambda g: seen.__setitem__("d_feat", g.detach().clone()))
        seen["feat"] = feat.detach()
        return feat

    monkeypatch.setattr(vc, "conv_stack_eval", spy)
    total, _vl, _al, _ent = agent.loss(sample_tuple(kind, s))
    agent.optimizer.zero_grad()
    total.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert seen["precision"] == "bf16"
    P = {k[len("base.imgCNN."):]: v for k, v in Q.items() if k.startswith("base.imgCNN.")}
    got, sv, gv = {"feat": host(seen["feat"])}, host(seen["saved"]), host(seen["gm"])
    for name, (off, shape) in seen["smap"].items():
        n = int(np.prod(shape))
        got["act." + name], got["g." + name] = sv[off:off + n].reshape(shape), gv[off:off + n].reshape(shape)
    grads = dict(pol.base.imgCNN.named_parameters())
    got.update({"d." + k: host(grads[k].grad) for k in cc.param_names(kind)})
    worst = parity(kind, P, {"image": s["image"], "d_feat": host(seen["d_feat"])}, got, cb.bounds(kind, T * N), f"kind {kind} PPO")
    print(f"kind {kind} PPO.loss through bind_convs(precision='bf16'): worst error / bound {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0, worst
    assert np.isfinite(float(total.detach()))
    for k, v in pol.named_parameters():
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()), k
    # the stacks ran in the mode: their output differs from the fp32 evaluation's, by a bf16 product's worth
    obs = sample_tuple(kind, s)[0]
    with torch.no_grad():
        f16 = var_amd.conv_stack_eval(pol.base.imgCNN, obs["image"], precision="bf16")
        f32 = var_amd.conv_stack_eval(pol.base.imgCNN, obs["image"])
    assert not torch.equal(f16, f32) and cb.rel(host(f16), host(f32)) < 0.05


@pytest.mark.parametrize("kind,n_act", [(0, 2), (1, 8)])
def test_one_fused_ppo_update_through_bf16_bind_convs_moves_the_arena_in_place(var_amd, kind, n_act):
    import types

    class Box:
        shape = (n_act,)

    class Discrete:
        n = n_act

    Q = cc.policy_params(kind, 9, n_act)
    pol = var_amd.bind_convs(real_policy(kind, Q), precision="bf16")
    flat, addr = pol._flat, pol._flat.data_ptr()
    before = flat.clone()
    shapes = {'image': (3, 96, 96), 'image_feat': (3,), 'goal_sound_feat': (3,)}
    shapes.update({'occupancy': (1, 9, 9)} if kind else {'robot_pose': (2,)})
    space = Discrete() if kind else Box()
    g, g_act = torch.Generator().manual_seed(4), torch.Generator().manual_seed(5)

    def observations(gen=g):
        return {k: (torch.randint(0, 256, (N,) + tuple(sh), generator=gen, dtype=torch.uint8) if k in ("image", "occupancy")
                    else torch.randn((N,) + tuple(sh), generator=gen)).cuda() for k, sh in shapes.items()}

    step = pol.capture(N, seed=0)                                    # an acting step captured BEFORE the update
    act_obs = observations(g_act)
    first = [t.clone() for t in step(act_obs, torch.ones(N, 1).cuda())]
    ro = var_amd.RolloutStorage(T, N, shapes, space, tc.hidden(kind), types.SimpleNamespace(RLObsIgnore=[]), image_dtype=torch.uint8)
    for _ in range(T):
        act = torch.randint(0, n_act, (N, 1), generator=g) if kind else torch.randn(N, n_act, generator=g)
        ro.insert(observations(), (0.5 * torch.randn(N, tc.hidden(kind), generator=g)).cuda(), act.cuda(),
                  (torch.randn(N, 1, generator=g) * 0.3 - 1.5).cuda(), torch.randn(N, 1, generator=g).cuda(), torch.randn(N, 1, generator=g).cuda(),
                  (torch.rand(N, 1, generator=g) < 0.8).float().cuda(), torch.ones(N, 1).cuda())
    ro.compute_returns(torch.randn(N, 1, generator=g).cuda(), True, 0.99, 0.95, True)
    agent = var_amd.PPO(pol, tc.CLIP, 1, 1, tc.VCOEF, tc.ECOEF, lr=1e-3, eps=1e-5, max_grad_norm=0.5, fused_optimizer=True)
    stats = agent.update(ro)
    torch.cuda.synchronize()
    assert all(np.isfinite(x) for x in stats), stats
    assert pol._flat is flat and flat.data_ptr() == addr and pol._arena_intact()
    moved = flat != before
    print(f"kind {kind}: stats {stats}, {int(moved.sum())} of {flat.numel()} arena floats moved")
    assert bool(torch.isfinite(flat).all()) and bool(moved.any())
    stack = pol.base.imgCNN.named_parameters()
    print(f"  imgCNN tensors moved: {[n for n, q in stack if bool((q.data != dev(Q['base.imgCNN.' + n])).any())]}")
    step.reset()                                                    # the captured step still replays, on the updated weights: the same
    out = step(act_obs, torch.ones(N, 1).cuda())                       # observations from the same hidden state give another value
    torch.cuda.synchronize()
    assert all(bool(torch.isfinite(t.float()).all()) for t in out) and len(first) == len(out)
    assert not torch.equal(out[0], first[0])

"""GPU checks of the actor-critics' convolution stacks (csrc/convstack.hip: var_convstack_fwd / var_convstack_bwd;
var_amd.conv_stack_eval / bind_convs) against the float64 checker of tests/convstack_cpu.py and the fixtures made from the
reference's Policy (tests/golden/convstack_*.npz).

Bounds are measured, not chosen (convstack_cpu.convstack_distance): per output, saved activation and gradient array four times
the distance of torch's own fp32 CPU evaluation from float64, the largest over the draws at the tested shape (20 up to B = 5, 3
beyond), relative to the array's largest magnitude; five such distances against the fixtures.  The float64 backward is taken at
the GPU's own ReLU gates and pool choices, and the units that differ from the float64 forward's are counted and must be near ties
(convstack_cpu's docstring).  Every test prints what it measured.  Determinism, graph replay and the extent of the writes are
bit for bit.

Batch sizes: 1, 2, 3, 5, 15, and both sides of every size at which a product's 128-row tile count first exceeds one -- 9 B pixels
of the image stacks' last maps (14 | 15), 25 B of kind 0's 5 x 5 map (5 | 6), 36 B of the parity classes of kind 0's stride-2 data
gradient (3 | 4) -- at which the weight gradient of a 25 B- or 9 B-pixel layer is first split in two (8 | 9, 24 | 25), and, for
kind 2, at which its weight gradients take another slab of eight images (8 | 9, 16 | 17, 24 | 25); kind 2 also at the update's 200
images, at the limit of 1024 (128 slabs) and one below it (a ragged 128th slab).  The form of a fold and the number of bias
partials depend on the layer alone.  The image stacks' larger batches are tests/test_gpu_convstack_large.py's."""
import ctypes

import numpy as np
import pytest
import torch

from tests import convstack_cpu as cc
from tests import trunk_cpu as tc

pytestmark = pytest.mark.gpu

BATCHES = {0: (1, 2, 3, 4, 5, 6, 8, 9, 14, 15, 24, 25), 1: (1, 2, 3, 5, 14, 15, 24, 25), 2: (1, 2, 3, 5, 6, 8, 9, 14, 15, 16, 17, 24, 25, 200, 1023, 1024)}
# uint8 images at every size, float images at three of them
CASES = [(k, B, True) for k in (0, 1, 2) for B in BATCHES[k]] + [(k, B, False) for k in (0, 1, 2) for B in (2, 5, 15)]
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


def run(var_amd, kind, P, d, module=None):
    """conv_stack_eval on the GPU, forward and backward: evaluate()'s arrays (no 'pre.*')."""
    module = cc.stack_module(kind, P).cuda() if module is None else module
    image = dev(d["image"])
    feat, saved, smap = var_amd.conv_stack_eval(module, image, return_saved=True)
    sv = host(saved)
    res = {"feat": host(feat)}
    for name, (off, shape) in smap.items():
        res["act." + name] = sv[off:off + int(np.prod(shape))].reshape(shape)
    params = dict(module.named_parameters())
    grads = torch.autograd.grad((feat * dev(d["d_feat"])).sum(), [params[k] for k in cc.param_names(kind)])
    res.update({"d." + k: host(g) for k, g in zip(cc.param_names(kind), grads)})
    assert np.array_equal(host(image), d["image"])                               # the input is unchanged
    return res


# ---- 1: forward, every saved activation and backward against float64; gates and pool choices ------------------------------------
@pytest.mark.parametrize("kind,B,u8", CASES)
def test_forward_saved_and_backward_match_float64(var_amd, kind, B, u8):
    dist = cc.convstack_distance(kind, B)
    seed = cc.find_seed(kind, B, cc.CASE_SEED)
    P, d, ref_fwd, _r32 = cc.case(kind, B, seed)
    if not u8:
        d = dict(d, image=cc.as_float_image(d["image"]))
    got = run(var_amd, kind, P, d)
    assert np.array_equal(bits(got["feat"]), bits(got["act." + cc.layer_names(kind)[-1]].reshape(B, -1)))     # the last map IS feat
    flips, ratio = cc.flipped_units(kind, got, ref_fwd, dist)
    units = sum(int(np.prod(s)) for s in cc.map_shapes(kind, B).values())
    print(f"kind {kind} B {B} {'u8' if u8 else 'f32'} seed {seed}: {flips} flipped gates / pool choices among {units} units, worst "
          f"margin / allowance {ratio:.3f}")
    assert flips <= cc.MAX_FLIPS and ratio <= 1.0, (flips, ratio)
    ref = cc.with_sums(cc.evaluate(kind, P, d, torch.float64, gates=cc.gates_of(got, kind), choices=cc.choices_of(got, kind)))
    got = cc.with_sums(got)
    assert set(got) == set(ref) == set(dist)
    worst = (0.0, None)
    for k in ref:
        err, bound = cc.rel(got[k], ref[k]), cc.MARGIN * dist[k]
        assert bound > 0 and np.abs(ref[k]).max() > 0, k
        worst = max(worst, (err / bound, (k, err, bound)))
    print(f"  worst error / bound {worst[0]:.3f} at {worst[1]}")
    if B > 5:
        cc.forget(kind, B)
    assert worst[0] <= 1.0, worst


# ---- 2: the fixtures made from the reference ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_fixture_from_the_reference(var_amd, golden_dir, kind):
    g = cc.load_fixture(golden_dir, kind)
    P, d = cc.fixture_inputs(kind, g)
    got = run(var_amd, kind, P, d)
    dist = cc.convstack_distance(kind, cc.FIXTURE_B)
    errs = cc.fixture_distances(kind, {k: v for k, v in got.items() if not k.startswith("act.")}, g)
    assert len(errs) == 1 + 4 * len(cc.layer_names(kind))
    worst = max((e / (cc.FIXTURE_MARGIN * dist[k]), k, e) for k, e in errs.items())
    print(f"kind {kind}: {len(errs)} arrays, worst error / bound {worst[0]:.3f} at {worst[1:]}")
    assert worst[0] <= 1.0, worst


# ---- 3: bit for bit ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1, 2])
def test_two_runs_give_equal_bits(var_amd, kind):
    B = 6
    P, d = cc.convstack_params(kind, 31), cc.convstack_data(kind, B, 31)
    module = cc.stack_module(kind, P).cuda()
    a, b = run(var_amd, kind, P, d, module), run(var_amd, kind, P, d, module)
    assert set(a) == set(b)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    # a float image holding the same numbers gives the same bits as the bytes
    c = run(var_amd, kind, P, dict(d, image=cc.as_float_image(d["image"])), module)
    for k in a:
        assert np.array_equal(bits(a[k]), bits(c[k])), k


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_forward_and_backward_replay_from_a_captured_graph(var_amd, kind):
    from var_amd._lib import new_graph
    B = 3
    P = cc.convstack_params(kind, 40)
    draws = [cc.convstack_data(kind, B, 40 + i) for i in range(3)]
    module = cc.stack_module(kind, P).cuda()
    eager = [run(var_amd, kind, P, d, module) for d in draws]
    static = {k: dev(draws[0][k]) for k in ("image", "d_feat")}
    params = dict(module.named_parameters())
    leaves = [params[k] for k in cc.param_names(kind)]
    g = new_graph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        feat = var_amd.conv_stack_eval(module, static["image"])
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


# ---- 4: the C ABI: extent of the writes, refused calls ------------------------------------------------------------------------------
def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Call:
    """Buffers of one var_convstack_fwd + var_convstack_bwd pair, every output inside a sentinel-filled buffer with PAD floats on
    each side."""
    PAD = 64

    def __init__(self, lib, kind, B, seed=3, u8=True):
        self.lib, self.kind, self.B, self.u8 = lib, kind, B, u8
        self.P, self.d = cc.convstack_params(kind, seed), cc.convstack_data(kind, B, seed, u8=u8)
        self.params = [dev(self.P[k]) for k in cc.param_names(kind)]
        self.table = (ctypes.c_void_p * len(self.params))(*(t.data_ptr() for t in self.params))
        self.inp = {k: dev(self.d[k]) for k in ("image", "d_feat")}
        self.n_saved = lib.var_convstack_saved_floats(kind, B)
        self.n_grad = lib.var_convstack_grad_offset(kind, len(self.params))
        self.ws_bytes = lib.var_convstack_workspace_bytes(kind, B)
        self.size = {"feat": B * cc.feat_width(kind), "saved": self.n_saved, "grads": self.n_grad, "ws": self.ws_bytes // 4}
        self.buf = {k: torch.full((n + 2 * self.PAD,), SENT, device="cuda") for k, n in self.size.items()}
        self.out = {k: b[self.PAD:self.PAD + self.size[k]] for k, b in self.buf.items()}
        self.bstride = int(np.prod(cc.STACKS[kind][0]))

    def _common(self, over):
        a = dict(kind=self.kind, params=self.table, image=p(self.inp["image"]), u8=int(self.u8), bstride=self.bstride, B=self.B,
                 feat=p(self.out["feat"]), saved=p(self.out["saved"]), d_feat=p(self.inp["d_feat"]), grads=p(self.out["grads"]),
                 ws=p(self.out["ws"]), ws_bytes=self.ws_bytes)
        a.update(over)
        return a

    def fwd(self, **over):
        from var_amd._lib import Context
        a = self._common(over)
        return self.lib.var_convstack_fwd(Context.get(0).handle, None, a["kind"], a["params"], a["image"], a["u8"], a["bstride"], a["B"],
                                          a["feat"], a["saved"], a["ws"], a["ws_bytes"])

    def bwd(self, **over):
        from var_amd._lib import Context
        a = self._common(over)
        return self.lib.var_convstack_bwd(Context.get(0).handle, None, a["kind"], a["params"], a["image"], a["u8"], a["bstride"], a["B"],
                                          a["saved"], a["d_feat"], a["grads"], a["ws"], a["ws_bytes"])

    def pads_intact(self):
        torch.cuda.synchronize()
        return all(bool((b[:self.PAD] == SENT).all()) and bool((b[self.PAD + self.size[k]:] == SENT).all()) for k, b in self.buf.items())

    def untouched(self, names):
        torch.cuda.synchronize()
        return all(bool((self.buf[k] == SENT).all()) for k in names)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_outputs_are_fully_overwritten_and_nothing_outside_them(var_amd, ctx, kind):
    from var_amd import convstack as vc
    B = 5
    c = Call(ctx.lib, kind, B)
    assert c.fwd() == 0, ctx.lib.var_last_error(ctx.handle)
    assert c.pads_intact() and c.untouched(("grads",))
    assert not bool((c.out["feat"] == SENT).any())
    covered = torch.zeros(c.n_saved, dtype=torch.bool, device="cuda")
    for name, (off, shape) in vc.saved_map(kind, B).items():
        n = int(np.prod(shape))
        assert not bool((c.out["saved"][off:off + n] == SENT).any()), name
        covered[off:off + n] = True
    assert bool(covered.all())                                       # (every offset is a multiple of four floats: no gaps)
    before = {k: c.out[k].clone() for k in ("feat", "saved")}
    assert c.bwd() == 0, ctx.lib.var_last_error(ctx.handle)
    assert c.pads_intact()
    for k in before:
        assert torch.equal(before[k], c.out[k]), k                   # the backward writes nothing the forward gave
    covered = torch.zeros(c.n_grad, dtype=torch.bool, device="cuda")
    for i, t in enumerate(c.params):
        off = ctx.lib.var_convstack_grad_offset(kind, i)
        assert not bool((c.out["grads"][off:off + t.numel()] == SENT).any()), cc.param_names(kind)[i]
        covered[off:off + t.numel()] = True
    assert bool(covered.all())
    # the inputs are unchanged, and the numbers are conv_stack_eval's
    assert np.array_equal(host(c.inp["image"]), c.d["image"]) and np.array_equal(host(c.inp["d_feat"]), c.d["d_feat"])
    for t, k in zip(c.params, cc.param_names(kind)):
        assert np.array_equal(host(t), c.P[k]), k
    got = run(var_amd, kind, c.P, c.d)
    assert np.array_equal(bits(host(c.out["feat"])), bits(got["feat"].ravel()))
    flat = np.concatenate([got["d." + k].ravel() for k in cc.param_names(kind)])
    assert np.array_equal(bits(host(c.out["grads"])), bits(flat))
    # a forward nobody differentiates (saved = NULL) gives the same output; images further apart than C*H*W too
    c2 = Call(ctx.lib, kind, B)
    assert c2.fwd(saved=None) == 0
    assert c2.pads_intact() and c2.untouched(("saved", "grads"))
    assert torch.equal(c2.out["feat"], c.out["feat"])
    wide = torch.zeros(B, c.bstride + 40, dtype=torch.uint8, device="cuda")
    wide[:, :c.bstride] = c.inp["image"].reshape(B, -1)
    c3 = Call(ctx.lib, kind, B)
    assert c3.fwd(image=p(wide), bstride=c.bstride + 40) == 0 and c3.bwd(image=p(wide), bstride=c.bstride + 40) == 0
    assert torch.equal(c3.out["feat"], c.out["feat"]) and torch.equal(c3.out["grads"], c.out["grads"])


def test_refused_calls_launch_nothing(ctx):
    lib = ctx.lib
    for kind in (0, 1, 2):
        c = Call(lib, kind, 2)
        null_table = (ctypes.c_void_p * len(c.params))(*([t.data_ptr() for t in c.params[:-1]] + [None]))
        common = [dict(B=0), dict(B=1025), dict(kind=3), dict(kind=-1), dict(params=null_table), dict(params=None),
                  dict(ws_bytes=c.ws_bytes - 1), dict(image=None), dict(ws=None), dict(bstride=c.bstride - 1)]
        for over in common + [dict(feat=None)]:
            assert c.fwd(**over) == -1, ("fwd", kind, over)
            assert lib.var_last_error(ctx.handle).decode().startswith("var_convstack_fwd"), over
        for over in common + [dict(saved=None), dict(d_feat=None), dict(grads=None)]:
            assert c.bwd(**over) == -1, ("bwd", kind, over)
            assert lib.var_last_error(ctx.handle).decode().startswith("var_convstack_bwd"), over
        assert c.untouched(("feat", "saved", "grads", "ws"))
        assert np.array_equal(host(c.inp["image"]), c.d["image"])
        assert c.fwd() == 0 and c.bwd() == 0                          # and a good pair right after the refused ones
        ref = cc.evaluate(kind, c.P, c.d, torch.float64)
        assert cc.rel(host(c.out["feat"]), ref["feat"].ravel()) < 1e-5
        off = lib.var_convstack_grad_offset(kind, 1)
        assert cc.rel(host(c.out["grads"][off:off + c.params[1].numel()]), ref["d." + cc.param_names(kind)[1]]) < 1e-4


def test_the_wrapper_refuses_before_any_launch(var_amd):
    module = cc.stack_module(0, cc.convstack_params(0, 1)).cuda()
    for image in (torch.zeros(2, 3, 96, 96), torch.zeros(2, 3, 96, 96, dtype=torch.float64, device="cuda"),
                  torch.zeros(2, 3, 84, 84, device="cuda"), torch.zeros(0, 3, 96, 96, device="cuda"),
                  torch.zeros(2, 3, 96, 96, device="cuda", requires_grad=True)):
        with pytest.raises(var_amd.VarHipError):
            var_amd.conv_stack_eval(module, image)
    with pytest.raises(var_amd.VarHipError):
        var_amd.conv_stack_eval(module.double(), torch.zeros(2, 3, 96, 96, device="cuda"))


# ---- 5: the binding ------------------------------------------------------------------------------------------------------------------
T, N = 3, 2


def real_policy(kind, Q):
    """An ArmNetPolicy / IthorNetPolicy with its own (real) convolution stacks, Q loaded, on the GPU."""
    pol = tc.drop_in_policy(kind, 0).to("cuda")                      # (Box(2) / Discrete(8))
    assert set(dict(pol.named_parameters())) == set(Q)
    with torch.no_grad():
        for k, v in pol.named_parameters():
            v.copy_(dev(Q[k]))
    assert pol._arena_intact()
    return pol


def sample_tuple(kind, s):
    obs = {k: dev(s[k]) for k in ("image", "image_feat", "goal_sound_feat") + (("occupancy",) if kind else ("robot_pose",))}
    return (obs,) + tuple(dev(s[k]) for k in ("hxs", "actions", "value_preds", "returns", "masks", "old_logp", "adv"))


def watch_stacks(kind, pol):
    """Forward hooks on the policy's convolution stacks as PyTorch runs them: (captured, remove) -- captured fills with every
    convolution's post-ReLU map (by parameter prefix) and the stacks' flattened outputs (by observation name) at the next forward."""
    captured, handles = {"acts": {}, "outs": {}}, []

    def keep(where, key):
        def hook(_mod, _inp, out):
            captured[where][key] = out.detach().clone()
        return hook

    for prefix, sk, name in cc.policy_stacks(kind):
        module = pol.base.occupancyCNNMLP if sk == 2 else pol.base.imgCNN
        for n in cc.layer_names(sk):
            handles.append(module[int(n) + 1].register_forward_hook(keep("acts", prefix + n)))          # the ReLU behind the convolution
        flatten = module[4] if sk == 2 else module[len(module) - 1]
        handles.append(flatten.register_forward_hook(keep("outs", name)))
    return captured, lambda: [h.remove() for h in handles]


def gpu_units(var_amd, kind, pol, s, captured=None):
    """The GPU's own gates and pool choices: the same ops on the same observations, with the saved activations.  captured: the
    stacks' maps and outputs as PyTorch computed them (watch_stacks), for a policy whose stacks run under PyTorch autograd."""
    from var_amd import convstack as vc
    acts = {}
    with torch.no_grad():
        obs = sample_tuple(kind, s)[0]
        outs = {}
        if captured is not None:
            acts.update({k: host(v) for k, v in captured["acts"].items()})
            outs = dict(captured["outs"])
            assert set(acts) == {prefix + n for prefix, sk, _name in cc.policy_stacks(kind) for n in cc.layer_names(sk)}
        else:
            for prefix, sk, name in cc.policy_stacks(kind):
                module = pol.base.occupancyCNNMLP if sk == 2 else pol.base.imgCNN
                outs[name], saved, smap = var_amd.conv_stack_eval(module, obs[name], return_saved=True)
                sv = host(saved)
                acts.update({prefix + n: sv[off:off + int(np.prod(shape))].reshape(shape) for n, (off, shape) in smap.items()})
        assert set(vc.saved_map(kind, T * N)) == set(cc.layer_names(kind))
        motor_in = obs["image_feat"] if kind else torch.cat([obs["image_feat"], obs["robot_pose"]], 1)
        *_, saved, smap = var_amd.trunk_eval(pol.base, outs["image"], motor_in, obs["goal_sound_feat"], dev(s["hxs"]), dev(s["masks"]),
                                             occ=outs.get("occupancy"), return_saved=True)
        sv = host(saved)
        acts.update({"base." + n: sv[off:off + rows * cols].reshape(rows, cols) for n, (off, rows, cols) in smap.items() if n != "gru.saved"})
    return cc.policy_units(kind, acts)


def ppo_loss_grads(var_amd, kind, n_act, binder, watch=False):
    """PPO.loss(sample).backward() through `binder`(policy) at the case's seed, against the float64 restatement at the gates and
    pool choices of THAT evaluation -- conv_stack_eval's saved maps, or with `watch` the maps PyTorch's own stacks produced in the
    very forward that is differentiated: the worst error / bound over the parameters."""
    dist = cc.ppo_distance(kind, T, N, n_act)
    seed = cc.find_ppo_seed(kind, T, N, n_act, cc.PPO_SEED)
    Q, s, _g64, a64, _g32, _a32 = cc.ppo_case(kind, T, N, n_act, seed)
    pol = real_policy(kind, Q)
    assert binder(pol) is pol
    with pytest.raises(NotImplementedError):
        pol.evaluate_actions(None, None, None, None)                 # (unchanged: PPO uses .base and .dist)
    agent = var_amd.PPO(pol, tc.CLIP, 1, 1, tc.VCOEF, tc.ECOEF, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    captured, remove = watch_stacks(kind, pol) if watch else (None, lambda: None)
    total, _vl, _al, _ent = agent.loss(sample_tuple(kind, s))
    remove()
    agent.optimizer.zero_grad()
    total.backward()
    got = {k: host(v.grad) for k, v in pol.named_parameters()}
    units = gpu_units(var_amd, kind, pol, s, captured)
    flips = cc.count_unit_flips(units, cc.policy_units(kind, a64))
    ref, _acts = cc.ppo_grads(kind, Q, s, torch.float64, *units)
    t64 = float(cc.ppo_total(kind, tc._tensors(Q, torch.float64), tc._tensors(s, torch.float64))[0])
    print(f"kind {kind} seed {seed}: total {float(total.detach()):.7f}, float64 {t64:.7f}, {flips} flipped gates / pool choices")
    assert abs(float(total.detach()) - t64) <= 1e-5 * max(1.0, abs(t64)) and flips <= cc.MAX_FLIPS
    assert set(got) == set(ref)
    worst = (0.0, None)
    for k in ref:
        assert np.abs(ref[k]).max() > 0, k
        err, bound = cc.rel(got[k], ref[k]), cc.MARGIN * dist[k]
        worst = max(worst, (err / bound, (k, err, bound)))
    return worst


@pytest.mark.parametrize("kind,n_act", [(0, 2), (1, 8)])
def test_ppo_loss_through_bind_convs_fills_every_gradient(var_amd, kind, n_act):
    worst = ppo_loss_grads(var_amd, kind, n_act, var_amd.bind_convs)
    print(f"  bind_convs: worst error / bound {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0, worst


@pytest.mark.parametrize("kind,n_act", [(0, 2), (1, 8)])
def test_ppo_loss_through_bind_trunk_is_within_the_same_bound(var_amd, kind, n_act):
    """The same policy with the stacks under PyTorch autograd (the one leg that may touch MIOpen), held to the same bound against
    the same float64 restatement -- at the gates and pool choices of ITS forward, read by hooks on the stacks' ReLUs.  (Against
    conv_stack_eval's gates this leg was 110 to 990 bounds off in its convolution weight gradients: with 6 images, one ReLU gate
    of the 5 x 5 map that falls the other way between two summation orders is one of a weight gradient's 150 terms.)"""
    worst = ppo_loss_grads(var_amd, kind, n_act, var_amd.bind_trunk, watch=True)
    print(f"  bind_trunk: worst error / bound {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0, worst


@pytest.mark.parametrize("kind,n_act", [(0, 2), (1, 8)])
def test_one_ppo_update_through_bind_convs_changes_the_arena_in_place(var_amd, kind, n_act):
    import types

    class Box:                                   # stand-ins for gym.spaces: the storage reads __class__.__name__ and .shape / .n
        shape = (n_act,)

    class Discrete:
        n = n_act

    Q = cc.policy_params(kind, 9, n_act)
    pol = var_amd.bind_convs(real_policy(kind, Q))
    flat, addr = pol._flat, pol._flat.data_ptr()
    before = flat.clone()
    shapes = {'image': (3, 96, 96), 'image_feat': (3,), 'goal_sound_feat': (3,)}
    shapes.update({'occupancy': (1, 9, 9)} if kind else {'robot_pose': (2,)})
    space = Discrete() if kind else Box()
    ro = var_amd.RolloutStorage(T, N, shapes, space, tc.hidden(kind), types.SimpleNamespace(RLObsIgnore=[]), image_dtype=torch.uint8)
    g = torch.Generator().manual_seed(4)
    for _ in range(T):
        obs = {k: (torch.randint(0, 256, (N,) + tuple(sh), generator=g, dtype=torch.uint8) if k in ("image", "occupancy")
                   else torch.randn((N,) + tuple(sh), generator=g)).cuda() for k, sh in shapes.items()}
        act = torch.randint(0, n_act, (N, 1), generator=g) if kind else torch.randn(N, n_act, generator=g)
        ro.insert(obs, (0.5 * torch.randn(N, tc.hidden(kind), generator=g)).cuda(), act.cuda(), (torch.randn(N, 1, generator=g) * 0.3 - 1.5).cuda(),
                  torch.randn(N, 1, generator=g).cuda(), torch.randn(N, 1, generator=g).cuda(), (torch.rand(N, 1, generator=g) < 0.8).float().cuda(),
                  torch.ones(N, 1).cuda())
    ro.compute_returns(torch.randn(N, 1, generator=g).cuda(), True, 0.99, 0.95, True)
    agent = var_amd.PPO(pol, tc.CLIP, 1, 1, tc.VCOEF, tc.ECOEF, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    stats = agent.update(ro)
    torch.cuda.synchronize()
    assert all(np.isfinite(x) for x in stats), stats
    assert pol._flat is flat and flat.data_ptr() == addr and pol._arena_intact()
    moved = (flat != before)
    print(f"kind {kind}: stats {stats}, {int(moved.sum())} of {flat.numel()} arena floats moved, largest step {float((flat - before).abs().max()):.3g}")
    # (no share of the arena is asked for: with six rows a ReLU unit that is dead in all of them leaves whole rows and columns of
    # the weight gradients zero -- four in ten of the Kuka policy's gradient elements in the float64 restatement at this shape)
    assert bool(torch.isfinite(flat).all()) and bool(moved.any())
    for name, prm in pol.named_parameters():
        assert prm.grad is not None and bool((prm.data != dev(Q[name])).any()), name

"""GPU checks of the PPO update's MLP trunk (csrc/trunk.hip: var_trunk_fwd / var_trunk_bwd; var_amd.trunk_eval / bind_trunk) against
the float64 checker of tests/trunk_cpu.py and the fixtures made from the reference's Policy (tests/golden/trunk_*_t7.npz).

Bounds are measured, not chosen (trunk_cpu.trunk_distance): per output, saved activation and gradient array four times the distance
of torch's own fp32 CPU evaluation from float64, the largest over 20 seeded draws at the tested shape, relative to the array's
largest magnitude (10 draws at 224 to 258 rows and 5 from 481, where a draw costs a second of host time); five such distances against
the fixtures.  The float64 backward is taken at the GPU's own ReLU gates, and the
units whose gate differs from the float64 forward's are counted and must lie within rounding of zero (trunk_cpu's docstring).
Every test prints what it measured.  Determinism, the GRU part, graph replay and the extent of the writes are bit for bit."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import trunk_cpu as tc

pytestmark = pytest.mark.gpu

SMALL_CASES = [(k, T, N) for k in (0, 1) for T, N in ((1, 1), (3, 2), (2, 17), (7, 5))] + [(0, 33, 4), (1, 1, 5)]      # 20 draws each
# the row counts on either side of a change of tiling in csrc/trunk.hip (trunk_cpu.THRESHOLD_SHAPES says which): 10 draws each up
# to 258 rows, 5 from 481
CASES = SMALL_CASES + [(k, T, N) for T, N in tc.THRESHOLD_SHAPES for k in (0, 1)]
VARIANTS = tuple(tc.VARIANTS)
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


def run(var_amd, kind, P, d, variants=("all",), base=None):
    """trunk_eval on the GPU: {variant: evaluate()'s arrays (no 'pre.*')}, one forward and one backward per variant."""
    base = tc.module_from_params(kind, P).cuda() if base is None else base
    t = {k: dev(d[k]) for k in tc.input_names(kind)}
    leaf_names = ["feat", "hxs"] + (["occ"] if kind else [])
    for k in leaf_names:
        t[k].requires_grad_()
    value, feats, h_T, saved, smap = var_amd.trunk_eval(base, t["feat"], t["motor_in"], t["sound_in"], t["hxs"], t["masks"],
                                                         occ=t.get("occ"), return_saved=True)
    sv = host(saved)
    common = {"value": host(value), "actor_features": host(feats), "h_T": host(h_T)}
    for name, (off, rows, cols) in smap.items():
        if name != "gru.saved":
            common["act." + name] = sv[off:off + rows * cols].reshape(rows, cols)
    params = dict(base.named_parameters())
    leaves = [t[k] for k in leaf_names] + [params[k] for k in tc.param_names(kind)]
    keys = ["d_" + k for k in leaf_names] + ["d." + k for k in tc.param_names(kind)]
    res = {}
    for v in variants:
        terms = [(o * dev(d[k])).sum() for o, k, u in zip((value, feats, h_T), ("d_value", "d_actor_features", "d_hT"), tc.VARIANTS[v]) if u]
        grads = torch.autograd.grad(sum(terms[1:], terms[0]), leaves, retain_graph=True, allow_unused=True)
        r = dict(common)
        for k, g in zip(keys, grads):
            assert g is not None, (v, k)
            r[k] = host(g)
        res[v] = r
    return res


def compare(kind, got, ref_fwd, ref, dist, margin, keys=None):
    """The worst error / bound over the compared arrays: forward arrays against the float64 forward, gradients against `ref`."""
    worst = (0.0, None)
    for k in keys or tc.compared_keys(ref):
        r = ref_fwd if k.startswith(("value", "actor_features", "h_T", "act.")) else ref
        err, bound = tc.rel(got[k], r[k]), margin * dist[k]
        worst = max(worst, (err / bound if bound else (0.0 if err == 0 else np.inf), (k, err, bound)))
    return worst


# ---- 1: forward, every saved activation and backward against float64 --------------------------------------------------------------
@pytest.mark.parametrize("kind,T,N", CASES)
def test_forward_saved_and_backward_match_float64(var_amd, kind, T, N):
    """Up to 132 rows, then (T, N) = (14, 16), (15, 15), (6, 43), (13, 37), (9, 57), (16, 62), (20, 50): 224, 225, 258, 481, 513, 992 and
    1000 rows, each the smallest with N <= 64 on one side of a switch -- the 32-row tile of product_tile<2> with a ragged last tile
    (from 225 rows for the J >= 1024 data gradients, 481 for J = 512, 897 for d_occ, 993 for J = 256), a second and a third pass of
    column_sums (from 257 and 513 rows), three and four environment blocks in the recurrent sequence (N = 37, 57).  The layers
    with J <= 128 change tile at 2017, 4065 and 8161 rows; those sizes are NOT run: a float64 reference of the recurrent sequence
    there takes far longer than a test may, and product_tile<2> is one piece of code for every layer."""
    seed = tc.find_seed(kind, T, N, 100 * (kind + 1) + T + N)
    P, d = tc.trunk_inputs(kind, T, N, seed)
    got = run(var_amd, kind, P, d, VARIANTS)
    gates = tc.gates_of(got["all"], kind)
    ref_fwd = tc.evaluate(kind, P, d, torch.float64)["all"]
    ref = tc.evaluate(kind, P, d, torch.float64, gates=gates, variants=VARIANTS)
    dist = tc.case_distance(kind, T, N)
    flips, ratio = tc.flipped_gates(kind, gates, ref_fwd, dist["all"])
    print(f"kind {kind} T {T} N {N} rows {T * N} seed {seed} draws {tc.draws(T, N)}: {flips} flipped gates, worst |pre-activation| / allowance {ratio:.3f}")
    assert flips <= tc.MAX_FLIPS and ratio <= 1.0, (flips, ratio)
    for v in VARIANTS:
        assert np.array_equal(bits(got[v]["h_T"]), bits(got[v]["act.gru"][-N:]))      # h_T IS the last step's rows
        worst = compare(kind, got[v], ref_fwd, ref[v], dist[v], tc.MARGIN)
        print(f"  {v}: worst error / bound {worst[0]:.3f} at {worst[1]}")
        assert worst[0] <= 1.0, (v, worst)


# ---- 2: the fixtures made from the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_fixture_from_the_reference(var_amd, golden_dir, kind):
    g = tc.load_fixture(golden_dir, kind)
    P, d = tc.fixture_inputs(kind, g)
    got = run(var_amd, kind, P, d, ("no_d_hT",))["no_d_hT"]
    dist = tc.trunk_distance(kind, tc.FIXTURE_T, tc.FIXTURE_N)["no_d_hT"]
    errs = tc.fixture_distances(kind, {k: v for k, v in got.items() if not k.startswith("act.")}, g)
    assert len(errs) == 3 + 2 + kind + len(tc.param_names(kind)) + 2 * (2 + len(tc.layers(kind)))
    worst = max((e / (tc.FIXTURE_MARGIN * dist[k]), k, e) for k, e in errs.items())
    print(f"kind {kind}: {len(errs)} arrays, worst error / bound {worst[0]:.3f} at {worst[1:]}")
    assert worst[0] <= 1.0, worst


# ---- 3: bit for bit -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [0, 1])
def test_two_runs_give_equal_bits_and_the_gru_part_is_masked_gru(var_amd, kind):
    T, N = 2, 17
    P, d = tc.trunk_inputs(kind, T, N, 31)
    base = tc.module_from_params(kind, P).cuda()
    a, b = run(var_amd, kind, P, d, VARIANTS, base), run(var_amd, kind, P, d, VARIANTS, base)
    for v in VARIANTS:
        assert set(a[v]) == set(b[v])
        for k in a[v]:
            assert np.array_equal(bits(a[v][k]), bits(b[v][k])), (v, k)
    gru = base.gru
    out, h_T = var_amd.masked_gru(dev(a["all"]["act.imgMotorMlp.2"]), dev(d["hxs"]), dev(d["masks"]), gru.weight_ih_l0, gru.weight_hh_l0,
                                  gru.bias_ih_l0, gru.bias_hh_l0)
    assert np.array_equal(bits(host(out)), bits(a["all"]["act.gru"])) and np.array_equal(bits(host(h_T)), bits(a["all"]["h_T"]))


@pytest.mark.parametrize("kind", [0, 1])
def test_a_longer_sequence_leaves_earlier_steps_untouched(var_amd, kind):
    """A step's output does not depend on later steps: steps 0 .. 13 (210 rows) of the T = 15, N = 15 call equal the T = 14 call on
    the same inputs cut to 14 steps, bit for bit, in both outputs and every saved activation.  (Both sizes run the forward on
    16-row tiles; the tile width is the float64 cases' business.)"""
    T, N, Tc = 15, 15, 14
    rows = Tc * N
    P, d = tc.trunk_inputs(kind, T, N, tc.find_seed(kind, T, N, 100 * (kind + 1) + T + N))
    cut = {k: (v if k in ("hxs", "d_hT") else v[:rows]) for k, v in d.items()}
    base = tc.module_from_params(kind, P).cuda()
    whole, part = run(var_amd, kind, P, d, base=base)["all"], run(var_amd, kind, P, cut, base=base)["all"]
    keys = [k for k in part if k in ("value", "actor_features") or k.startswith("act.")]
    assert len(keys) == 2 + len(tc.layers(kind)) + 1
    for k in keys:
        assert part[k].shape[0] == rows and whole[k].shape[0] == T * N, k
        assert np.array_equal(bits(whole[k][:rows]), bits(part[k])), k
    assert not np.array_equal(whole["h_T"], part["h_T"])            # (the fifteenth step did run)


@pytest.mark.parametrize("kind", [0, 1])
def test_forward_and_backward_replay_from_a_captured_graph(var_amd, kind):
    from var_amd._lib import new_graph
    T, N = 3, 2
    draws = [tc.trunk_inputs(kind, T, N, 40 + i) for i in range(3)]
    base = tc.module_from_params(kind, draws[0][0]).cuda()
    eager = [run(var_amd, kind, P, d, ("all",), base)["all"] for P, d in [(draws[0][0], dd) for _, dd in draws]]
    names = tc.input_names(kind) + ("d_value", "d_actor_features", "d_hT")
    static = {k: dev(draws[0][1][k]) for k in names}
    leaf_names = ["feat", "hxs"] + (["occ"] if kind else [])
    params = dict(base.named_parameters())
    leaves = [static[k].requires_grad_() for k in leaf_names] + [params[k] for k in tc.param_names(kind)]
    keys = ["d_" + k for k in leaf_names] + ["d." + k for k in tc.param_names(kind)]
    g = new_graph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        value, feats, h_T = var_amd.trunk_eval(base, static["feat"], static["motor_in"], static["sound_in"], static["hxs"], static["masks"],
                                               occ=static.get("occ"))
        obj = (value * static["d_value"]).sum() + (feats * static["d_actor_features"]).sum() + (h_T * static["d_hT"]).sum()
        grads = torch.autograd.grad(obj, leaves)
    torch.cuda.current_stream().wait_stream(side)
    for i in (1, 2):
        with torch.no_grad():
            for k in names:
                static[k].copy_(dev(draws[i][1][k]))
        g.replay()
        got = {"value": host(value), "actor_features": host(feats), "h_T": host(h_T)}
        got.update({k: host(v) for k, v in zip(keys, grads)})
        for k in got:
            assert np.array_equal(bits(got[k]), bits(eager[i][k])), (i, k)


# ---- 4: the C ABI: extent of the writes, refused calls ----------------------------------------------------------------------------------
def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class Call:
    """Buffers of one var_trunk_fwd + var_trunk_bwd pair, every output inside a sentinel-filled buffer with PAD floats on each side."""
    PAD = 64

    def __init__(self, lib, kind, T, N, seed=3):
        self.lib, self.kind, self.T, self.N = lib, kind, T, N
        M, H = T * N, tc.hidden(kind)
        P, d = tc.trunk_inputs(kind, T, N, seed)
        self.P, self.d = P, d
        self.params = [dev(P[k]) for k in tc.param_names(kind)]
        self.table = (ctypes.c_void_p * len(self.params))(*(t.data_ptr() for t in self.params))
        self.inp = {k: dev(d[k]) for k in tc.input_names(kind) + ("d_value", "d_actor_features", "d_hT")}
        self.n_saved = lib.var_trunk_saved_floats(kind, T, N)
        self.n_grad = lib.var_trunk_grad_offset(kind, len(self.params))
        self.ws_bytes = lib.var_trunk_workspace_bytes(kind, T, N)
        sizes = {"value": M, "actor_features": M * 128, "h_T": N * H, "saved": self.n_saved, "d_feat": M * 1152, "d_occ": M * 288,
                 "d_hxs": N * H, "d_params": self.n_grad, "ws": self.ws_bytes // 4}
        self.size = sizes
        self.buf = {k: torch.full((n + 2 * self.PAD,), SENT, device="cuda") for k, n in sizes.items()}
        self.out = {k: b[self.PAD:self.PAD + sizes[k]] for k, b in self.buf.items()}

    def fwd(self, **over):
        a = dict(kind=self.kind, params=self.table, feat=p(self.inp["feat"]), occ=p(self.inp.get("occ")), motor_in=p(self.inp["motor_in"]),
                 sound_in=p(self.inp["sound_in"]), hxs=p(self.inp["hxs"]), masks=p(self.inp["masks"]), T=self.T, N=self.N,
                 value=p(self.out["value"]), actor_features=p(self.out["actor_features"]), h_T=p(self.out["h_T"]), saved=p(self.out["saved"]),
                 ws=p(self.out["ws"]), ws_bytes=self.ws_bytes)
        a.update(over)
        from var_amd._lib import Context
        return self.lib.var_trunk_fwd(Context.get(0).handle, None, a["kind"], a["params"], a["feat"], a["occ"], a["motor_in"], a["sound_in"],
                                      a["hxs"], a["masks"], a["T"], a["N"], a["value"], a["actor_features"], a["h_T"], a["saved"], a["ws"],
                                      a["ws_bytes"])

    def bwd(self, **over):
        a = dict(kind=self.kind, params=self.table, feat=p(self.inp["feat"]), occ=p(self.inp.get("occ")), motor_in=p(self.inp["motor_in"]),
                 sound_in=p(self.inp["sound_in"]), masks=p(self.inp["masks"]), T=self.T, N=self.N, saved=p(self.out["saved"]),
                 d_value=p(self.inp["d_value"]), d_actor_features=p(self.inp["d_actor_features"]), d_hT=p(self.inp["d_hT"]),
                 d_feat=p(self.out["d_feat"]), d_occ=p(self.out["d_occ"]) if self.kind else None, d_hxs=p(self.out["d_hxs"]),
                 d_params=p(self.out["d_params"]), ws=p(self.out["ws"]), ws_bytes=self.ws_bytes)
        a.update(over)
        from var_amd._lib import Context
        return self.lib.var_trunk_bwd(Context.get(0).handle, None, a["kind"], a["params"], a["feat"], a["occ"], a["motor_in"], a["sound_in"],
                                      a["masks"], a["T"], a["N"], a["saved"], a["d_value"], a["d_actor_features"], a["d_hT"], a["d_feat"],
                                      a["d_occ"], a["d_hxs"], a["d_params"], a["ws"], a["ws_bytes"])

    def pads_intact(self):
        torch.cuda.synchronize()
        return all(bool((b[:self.PAD] == SENT).all()) and bool((b[self.PAD + self.size[k]:] == SENT).all()) for k, b in self.buf.items())

    def untouched(self, names):
        torch.cuda.synchronize()
        return all(bool((self.buf[k] == SENT).all()) for k in names)


class Box:                                   # stand-ins for gym.spaces: the storage reads __class__.__name__ and .shape / .n
    def __init__(self, n):
        self.shape = (n,)


class Discrete:
    def __init__(self, n):
        self.n = n


FWD_OUT, BWD_OUT = ("value", "actor_features", "h_T", "saved"), ("d_feat", "d_occ", "d_hxs", "d_params")


@pytest.mark.parametrize("kind", [0, 1])
def test_outputs_are_fully_overwritten_and_nothing_outside_them(var_amd, ctx, kind):
    from var_amd import trunk as vt
    T, N = 2, 17
    c = Call(ctx.lib, kind, T, N)
    assert c.fwd() == 0, ctx.lib.var_last_error(ctx.handle)
    assert c.pads_intact() and c.untouched(BWD_OUT)
    for k in ("value", "actor_features", "h_T"):
        assert not bool((c.out[k] == SENT).any()), k
    smap = vt.saved_map(kind, T, N)
    covered = torch.zeros(c.n_saved, dtype=torch.bool, device="cuda")
    for name, (off, rows, cols) in smap.items():
        assert not bool((c.out["saved"][off:off + rows * cols] == SENT).any()), name
        covered[off:off + rows * cols] = True
    assert bool((c.out["saved"][~covered] == SENT).all())          # the alignment gaps between the slices stay as they were
    before = {k: c.out[k].clone() for k in FWD_OUT}
    assert c.bwd() == 0, ctx.lib.var_last_error(ctx.handle)
    assert c.pads_intact()
    for k in FWD_OUT:
        assert torch.equal(before[k], c.out[k]), k                   # the backward writes nothing the forward gave
    for k in ("d_feat", "d_hxs") + (("d_occ",) if kind else ()):
        assert not bool((c.out[k] == SENT).any()), k
    if not kind:
        assert c.untouched(("d_occ",))
    covered = torch.zeros(c.n_grad, dtype=torch.bool, device="cuda")
    for i, t in enumerate(c.params):
        off = ctx.lib.var_trunk_grad_offset(kind, i)
        assert not bool((c.out["d_params"][off:off + t.numel()] == SENT).any()), tc.param_names(kind)[i]
        covered[off:off + t.numel()] = True
    assert bool((c.out["d_params"][~covered] == SENT).all())
    # and the numbers are trunk_eval's
    got = run(var_amd, kind, c.P, c.d)["all"]
    assert np.array_equal(bits(host(c.out["value"])), bits(got["value"].ravel()))
    assert np.array_equal(bits(host(c.out["d_feat"])), bits(got["d_feat"].ravel()))
    # a forward nobody differentiates (saved = NULL) gives the same outputs
    c2 = Call(ctx.lib, kind, T, N)
    assert c2.fwd(saved=None) == 0
    assert c2.pads_intact() and c2.untouched(("saved",) + BWD_OUT)
    for k in ("value", "actor_features", "h_T"):
        assert torch.equal(c2.out[k], c.out[k]), k


def test_refused_calls_launch_nothing(ctx):
    lib = ctx.lib
    for kind in (0, 1):
        c = Call(lib, kind, 2, 3)
        every = FWD_OUT + BWD_OUT + ("ws",)
        short = c.ws_bytes - 256
        null_table = (ctypes.c_void_p * len(c.params))(*([t.data_ptr() for t in c.params[:-1]] + [None]))
        fwd_bad = [dict(kind=2), dict(kind=-1), dict(N=0), dict(N=65), dict(T=0), dict(T=16385, N=1), dict(T=6000, N=3),
                   dict(feat=None), dict(motor_in=None), dict(sound_in=None), dict(hxs=None), dict(masks=None), dict(value=None),
                   dict(actor_features=None), dict(h_T=None), dict(ws=None), dict(params=None), dict(params=null_table),
                   dict(ws_bytes=short), dict(value=p(c.inp["masks"])), dict(h_T=p(c.inp["hxs"])), dict(actor_features=p(c.out["saved"]))]
        bwd_bad = [dict(kind=2), dict(N=0), dict(N=65), dict(T=0), dict(T=6000, N=3), dict(feat=None), dict(masks=None), dict(saved=None),
                   dict(d_feat=None), dict(d_hxs=None), dict(d_params=None), dict(ws=None), dict(params=null_table), dict(ws_bytes=short),
                   dict(d_feat=p(c.inp["feat"])), dict(d_hxs=p(c.inp["d_hT"])), dict(d_params=p(c.out["saved"]))]
        if kind:
            fwd_bad.append(dict(occ=None))
            bwd_bad += [dict(occ=None), dict(d_occ=None)]
        for over in fwd_bad:
            assert c.fwd(**over) == -1, ("fwd", kind, over)
            assert lib.var_last_error(ctx.handle).decode().startswith("var_trunk_fwd"), over
        for over in bwd_bad:
            assert c.bwd(**over) == -1, ("bwd", kind, over)
            assert lib.var_last_error(ctx.handle).decode().startswith("var_trunk_bwd"), over
        assert c.untouched(every)
        for k in ("feat", "hxs", "masks", "d_hT"):
            assert np.array_equal(host(c.inp[k]), c.d[k]), k
        assert c.fwd() == 0 and c.bwd() == 0                        # and a good pair right after the refused ones
        ref = tc.evaluate(kind, c.P, c.d, torch.float64)["all"]
        assert tc.rel(host(c.out["value"]), ref["value"]) < 1e-5


# ---- 5: the binding ---------------------------------------------------------------------------------------------------------------------
def bound_policy(var_amd, kind, Q, n_act):
    """An ArmNetPolicy / IthorNetPolicy with stand-in convolution stacks, Q loaded, on the GPU, bound."""
    pol = tc.drop_in_policy(kind, 0)                             # (Box(2) / Discrete(8))
    cnn, occ = tc.standin_modules(kind)
    pol.base.imgCNN = cnn
    if kind:
        pol.base.occupancyCNNMLP = nn.Sequential(*occ, *list(pol.base.occupancyCNNMLP)[5:])
    pol = pol.to("cuda")
    assert set(dict(pol.named_parameters())) == set(Q)
    with torch.no_grad():
        for k, v in pol.named_parameters():
            v.copy_(dev(Q[k]))
    assert pol._arena_intact()
    assert var_amd.bind_trunk(pol) is pol
    return pol


def sample_tuple(kind, s):
    obs = {k: dev(s[k]) for k in ("image", "image_feat", "goal_sound_feat") + (("occupancy",) if kind else ("robot_pose",))}
    return (obs,) + tuple(dev(s[k]) for k in ("hxs", "actions", "value_preds", "returns", "masks", "old_logp", "adv"))


@pytest.mark.parametrize("kind,n_act", [(0, 2), (1, 8)])
def test_ppo_loss_through_a_bound_policy_fills_every_gradient(var_amd, kind, n_act):
    T, N = 3, 2
    seed = tc.find_ppo_seed(kind, T, N, n_act, 50)
    Q = tc.standin_params(kind, seed, n_act)
    s = tc.ppo_sample(kind, Q, T, N, n_act, seed + 500)
    pol = bound_policy(var_amd, kind, Q, n_act)
    with pytest.raises(NotImplementedError):
        pol.evaluate_actions(None, None, None, None)                 # (unchanged: PPO uses .base and .dist)
    agent = var_amd.PPO(pol, tc.CLIP, 1, 1, tc.VCOEF, tc.ECOEF, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    total, _vl, _al, _ent = agent.loss(sample_tuple(kind, s))
    agent.optimizer.zero_grad()
    total.backward()
    # the GPU's own gates: the same trunk_eval on the same features, with the saved activations
    with torch.no_grad():
        obs = sample_tuple(kind, s)[0]
        feat = pol.base.imgCNN(obs["image"].float() / 255.0)
        occ = None
        if kind:
            occ = obs["occupancy"].float() / 255.0
            for mod in list(pol.base.occupancyCNNMLP)[:5]:
                occ = mod(occ)
        motor_in = obs["image_feat"] if kind else torch.cat([obs["image_feat"], obs["robot_pose"]], 1)
        *_, saved, smap = var_amd.trunk_eval(pol.base, feat, motor_in, obs["goal_sound_feat"], dev(s["hxs"]), dev(s["masks"]), occ=occ,
                                             return_saved=True)
    sv = host(saved)
    gates = {name: sv[off:off + rows * cols].reshape(rows, cols) > 0 for name, (off, rows, cols) in smap.items()
             if name in {n for n, *_r, relu in tc.layers(kind) if relu}}
    ref, acts = tc.ppo_grads(kind, Q, s, torch.float64, gates=gates)
    t64 = float(tc.ppo_total(kind, tc._tensors(Q, torch.float64), tc._tensors(s, torch.float64))[0])
    flips = sum(int(((acts["act." + k] > 0) != g).sum()) for k, g in gates.items())
    print(f"kind {kind} seed {seed}: total {float(total.detach()):.7f}, float64 {t64:.7f}, {flips} flipped gates")
    assert abs(float(total.detach()) - t64) <= 1e-5 * max(1.0, abs(t64)) and flips <= tc.MAX_FLIPS
    dist = tc.ppo_distance(kind, T, N, n_act)
    got = {k: v.grad for k, v in pol.named_parameters()}
    assert set(got) == set(ref)
    worst = (0.0, None)
    for k in ref:
        assert got[k] is not None, k
        err, bound = tc.rel(host(got[k]), ref[k]), tc.MARGIN * dist[k]
        worst = max(worst, (err / bound, (k, err, bound)))
        assert np.abs(ref[k]).max() > 0, k
    print(f"  worst error / bound {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0, worst


@pytest.mark.parametrize("kind,n_act", [(0, 2), (1, 8)])
def test_one_ppo_update_changes_the_arena_in_place(var_amd, kind, n_act):
    import types
    T, N = 3, 2
    Q = tc.standin_params(kind, 9, n_act)
    pol = bound_policy(var_amd, kind, Q, n_act)
    flat, addr = pol._flat, pol._flat.data_ptr()
    before = flat.clone()
    shapes = {'image': tc.IMAGE, 'image_feat': (3,), 'goal_sound_feat': (3,)}
    shapes.update({'occupancy': tc.OCC} if kind else {'robot_pose': (2,)})
    space = Discrete(n_act) if kind else Box(n_act)
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
    assert bool(torch.isfinite(flat).all()) and float(moved.float().mean()) > 0.5
    for name, prm in pol.named_parameters():
        assert prm.grad is not None and bool((prm.data != dev(Q[name])).any()), name

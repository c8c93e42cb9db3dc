"""The acting forwards with bf16 operands (var_armnet_forward_ex / var_ithor_policy_forward_ex flags bit 0; policy.set_acting_precision,
capture(precision=...)): every imgCNN convolution computes relu(conv(bf16(x), bf16(w)) + b) with fp32 accumulation, everything
stored stays fp32, everything behind the convolutions is the fp32 forward's.

1  Layer by layer on every route (B = 1, 3, 8, 9, 64, 65), both policies: each surviving buffer against float64 ON ROUNDED OPERANDS
   (tests/acting_bf16_cpu.py) evaluated from the device's own upstream buffers, bound MARGIN x the distance of torch's fp32 CPU
   evaluation of the same rounded function from float64 (never the kernel); the buffers that do not depend on the image equal the
   fp32 entry's bit for bit.  tests/test_acting_bf16_host.py shows that a convolution that forgot to round fails these checks.
2  _ex(..., 0) leaves the old entry's bits in every buffer.     3  Other flag bits are refused and nothing is written.
4  Determinism; a captured bf16 step replays the eager bf16 act's bits, picks up an in-place weight update, and an fp32 and a bf16
   step captured on one policy and plan replay side by side.
5  Acting against evaluation, the point of the mode: value and head of the bf16 acting forward and of bind_convs(precision="bf16")
   evaluation of the same rows each within MARGIN x the fp32-against-float64 distance of the whole rounded graph, within twice
   that of each other, and closer to each other than the fp32 acting forward is to the bf16 evaluation."""
import functools

import pytest
import torch

from tests import acting_bf16_cpu as ab
from tests import acting_layers_cpu as al
from tests import test_gpu_acting_layers as gl      # its helpers: read_back, obs_of, device_inputs (no test of it is imported)
from tests import trunk_cpu as tc

pytestmark = pytest.mark.gpu

MODELS = ("arm", "ipol")
N_ACT = {"arm": 2, "ipol": 8}
BATCHES = (1, 3, 8, 9, 64, 65)
BF16 = 1


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return m


def fresh_policy(model, seed=9):
    kind = ab.KIND[model]
    P = ab.policy_tensors(kind, seed, N_ACT[model])
    m = tc.drop_in_policy(kind, 0).to("cuda")
    assert set(dict(m.named_parameters())) == set(P)
    with torch.no_grad():
        for k, v in m.named_parameters():
            v.copy_(P[k].cuda())
    assert m._arena_intact() and m.acting_precision == "fp32"
    return m, P


@functools.lru_cache(maxsize=None)
def policy(model):
    """(the policy on the device with convstack_cpu.policy_params weights, those weights on the host); shared, never modified."""
    return fresh_policy(model)


def call(m, model, dev, outs, flags=0, ex=True):
    """The C entry itself (the old one, or _ex with `flags`) on device tensors; outs: value, feats, head, hout.  Returns rc."""
    from var_amd._lib import Context, ptr
    c = Context.get(0)
    image, B = dev["image"], dev["image"].shape[0]
    m._ensure_plan(c, B)
    value, feats, head, hout = outs
    tail = [ptr(dev["hxs"]), ptr(dev["masks"]), B, ptr(value), ptr(feats), ptr(head), ptr(hout)] + ([int(flags)] if ex else [])
    u8 = int(image.dtype == torch.uint8)
    if model == "arm":
        fn = c.lib.var_armnet_forward_ex if ex else c.lib.var_armnet_forward
        rc = fn(c.handle, None, ptr(m._flat), ptr(image), u8, image.stride(0), ptr(dev["image_feat"]), ptr(dev["robot_pose"]),
                ptr(dev["goal"]), *tail)
    else:
        fn = c.lib.var_ithor_policy_forward_ex if ex else c.lib.var_ithor_policy_forward
        occ = dev["occupancy"]
        rc = fn(c.handle, None, ptr(m._flat), m.n_actions, ptr(image), u8, image.stride(0), ptr(occ), int(occ.dtype == torch.uint8),
                ptr(dev["image_feat"]), ptr(dev["goal"]), *tail)
    torch.cuda.synchronize()
    return rc


def outputs(m, B, fill=float("nan")):
    out = lambda n: torch.full((B, n), fill, device="cuda")      # noqa: E731
    return out(1), out(128), out(m._n_head), out(m.recurrent_hidden_state_size)


def forward(m, model, dev, flags=0, ex=True):
    """One forward, then every buffer it left behind on the host (test_gpu_acting_layers.read_back)."""
    from var_amd._lib import Context
    B = dev["image"].shape[0]
    outs = outputs(m, B)
    rc = call(m, model, dev, outs, flags, ex)
    Context.get(0).check(rc, "forward")
    got = dict(zip(("value", "feats", "head", "hout"), outs))
    return gl.read_back(model, B, m.recurrent_hidden_state_size, got)


def case_inputs(model, B):
    inputs = al.random_inputs(model, B, 50 + B, u8=(B != 9))
    if B == 3:      # one saturated and one empty image beside the random one: the zero halo and the zero rows
        inputs["image"][0] = 255
        inputs["image"][1] = 0
    return inputs


def upstream_of_image(model):
    """The buffers of the graph that depend on the image."""
    G, memo = al.graph(model), {}

    def dep(k):
        if k not in memo:
            memo[k] = k == "image" or (k in G and any(dep(i) for i in G[k].ins))
        return memo[k]
    return {k for k in G if dep(k)}


def tensors_equal(a, b, keys=None):
    keys = [k for k in a if torch.is_tensor(a[k])] if keys is None else keys
    return [k for k in keys if not torch.equal(a[k], b[k])]


# ---- 1: layer by layer ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", BATCHES)
@pytest.mark.parametrize("model", MODELS)
def test_every_layer_against_float64_on_rounded_operands(var_amd, model, B):
    m, P = policy(model)
    inputs = case_inputs(model, B)
    dev = gl.device_inputs(inputs)
    f32 = forward(m, model, dev, 0)
    b = forward(m, model, dev, BF16)
    keep = al.survivors(model, B)
    images = [0, 1, B - 2, B - 1] if B >= 64 else None
    env = dict(inputs, **{k: b[k] for k in keep})
    tag = f"{model} B {B}"
    with torch.no_grad():
        res = ab.check_layers(model, env, P, keep, images=images, order=ab.order_for(model, B), log=lambda s: print(f"{tag}: {s}"))
    assert list(res) == keep
    maps = [k for k in keep if k in al.MAPS[model] and k != "occf"]
    want = {"arm": ["a1", "p1", "a3", "p2", "a5", "p3", "a7", "a8"], "ipol": ["a1", "p1", "p2", "p3", "p4", "a6"]}[model]
    assert maps == (want if B <= al.BAND_MAX_B else [k for k in al.MAPS[model] if k != "occf"])
    bad = [(k, r) for k, r in res.items() if not r[3] <= 1]                    # (not "any ratio > 1": a NaN must not pass)
    inexact = [k for k in keep if (k == "h0" or (k.startswith("p") and B > al.BAND_MAX_B)) and res[k][2] != 0]
    assert not inexact, inexact                                                # routing and selection: distance 0, bound 0
    assert not bad, bad
    # the mode ran in every convolution (each map differs from the fp32 forward's), and touched nothing that does not read the image
    assert not [k for k in maps if torch.equal(b[k], f32[k])]
    rest = [k for k in keep if k not in upstream_of_image(model) and k in f32]
    assert ("occf" in rest) == (model == "ipol") and "gh" in rest
    assert not tensors_equal(b, f32, rest)
    assert m.chain_status() == 0


# ---- 2: fp32 untouched ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", (8, 9))
@pytest.mark.parametrize("model", MODELS)
def test_flags_zero_leaves_the_old_entrys_bits(var_amd, model, B):
    m, _P = policy(model)
    dev = gl.device_inputs(al.random_inputs(model, B, 70 + B))
    old = forward(m, model, dev, ex=False)
    new = forward(m, model, dev, 0)
    assert set(old) == set(new) and not tensors_equal(old, new)
    assert bool(torch.isfinite(new["value"]).all()) and tensors_equal(new, forward(m, model, dev, BF16), ["value", "head"])


# ---- 3: refusals ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_other_flag_bits_are_refused_and_nothing_is_written(var_amd, model):
    from var_amd._lib import Context
    m, _P = policy(model)
    ctx = Context.get(0)
    dev = gl.device_inputs(al.random_inputs(model, 2, 81))
    name = "var_armnet_forward_ex" if model == "arm" else "var_ithor_policy_forward_ex"
    for flags in (2, 3, -2, 1 << 8):
        outs = outputs(m, 2, fill=-77.0)
        assert call(m, model, dev, outs, flags) == -1, flags                   # VAR_ERR_ARG
        assert ctx.lib.var_last_error(ctx.handle).decode().startswith(name), flags
        assert all(bool((t == -77.0).all()) for t in outs), flags
    outs = outputs(m, 2, fill=-77.0)
    assert call(m, model, dev, outs, BF16) == 0                                # and a good call right after the refused ones
    assert all(bool(torch.isfinite(t).all()) and not bool((t == -77.0).any()) for t in outs)


# ---- 4: determinism and capture ---------------------------------------------------------------------------------------------------------
def eager_act(m, model, dev, noise, precision):
    """policy's eager forward at `precision`, then var_policy_dist fed `noise`: (value, action, logp, hout, head)."""
    from var_amd._lib import Context, ptr
    c = Context.get(0)
    B = dev["image"].shape[0]
    before = m.acting_precision
    m.set_acting_precision(precision)
    try:
        value, _feats, head, hout = m._base_forward(gl.obs_of(model, dev), dev["hxs"], dev["masks"])
    finally:
        m.set_acting_precision(before)
    kind, n, _hidden, logstd, _shapes = m._step_spec(B, torch.uint8)
    action = torch.zeros(B, n, device="cuda") if kind == 0 else torch.zeros((B, 1), dtype=torch.int64, device="cuda")
    logp, used = torch.zeros(B, 1, device="cuda"), torch.zeros_like(noise)
    c.check(c.lib.var_policy_dist(c.handle, None, kind, ptr(head), ptr(logstd), n, B, 0, ptr(noise), None, ptr(used), ptr(action),
                                  ptr(logp), None, None, 0), "var_policy_dist")
    torch.cuda.synchronize()
    return value, action, logp, hout, head


def replay(step, model, dev):
    step.reset(dev["hxs"])
    value, action, logp, hout = step(gl.obs_of(model, dev), dev["masks"])
    torch.cuda.synchronize()
    return [t.clone() for t in (value, action, logp, hout, step.head)], step.noise.clone()


@pytest.mark.parametrize("model", MODELS)
def test_two_bf16_forwards_leave_equal_bits(var_amd, model):
    m, _P = policy(model)
    dev = gl.device_inputs(al.random_inputs(model, 8, 91))
    a, b = forward(m, model, dev, BF16), forward(m, model, dev, BF16)
    assert not tensors_equal(a, b, [k for k in a if torch.is_tensor(a[k])])
    assert bool(torch.isfinite(a["value"]).all())


@pytest.mark.parametrize("model", MODELS)
def test_captured_steps_in_both_precisions_replay_the_eager_bits_and_see_updated_weights(var_amd, model):
    m, _P = fresh_policy(model)                                                # (its weights change below)
    B = 8
    dev = gl.device_inputs(al.random_inputs(model, B, 93))
    s16 = m.capture(B, seed=5, precision="bf16")
    s32 = m.capture(B, seed=5)
    assert s16.precision == "bf16" and s32.precision == "fp32" and m.acting_precision == "fp32"
    m.set_acting_precision("bf16")
    assert m.capture(B, seed=5).precision == "bf16"                            # capture follows the policy's setting
    m.set_acting_precision("fp32")

    def both():
        outs = {}
        for prec, step in (("bf16", s16), ("fp32", s32), ("bf16 again", s16)):     # one after the other on one plan
            got, noise = replay(step, model, dev)
            want = eager_act(m, model, dev, noise, prec.split()[0])
            names = ("value", "action", "logp", "hout", "head")
            diff = [n for n, g, w in zip(names, got, want) if not torch.equal(g, w)]
            assert not diff, (prec, diff)
            outs[prec] = got
        assert not torch.equal(outs["bf16"][4], outs["fp32"][4])                # the two steps compute different functions
        assert torch.equal(outs["bf16"][4], outs["bf16 again"][4]) and torch.equal(outs["bf16"][0], outs["bf16 again"][0])
        return outs

    first = both()
    with torch.no_grad():
        m.base.imgCNN[2].weight.mul_(1.25)                                     # in place: the arena stays where it is
    assert m._arena_intact()
    second = both()                                                            # each replay equals a fresh eager call
    assert not torch.equal(first["bf16"][4], second["bf16"][4]) and not torch.equal(first["fp32"][4], second["fp32"][4])
    assert m.chain_status() == 0


# ---- 5: acting against evaluation -------------------------------------------------------------------------------------------------------
DRAWS = (101, 102, 103)


@pytest.mark.parametrize("model", MODELS)
def test_bf16_acting_and_bf16_evaluation_compute_one_function(var_amd, model):
    N = 4
    m, P = fresh_policy(model)                                                 # (bind_convs gives its base a forward)
    with torch.no_grad():
        drawn = [(al.random_inputs(model, N, s),) + ab.end_to_end_distance(model, P, al.random_inputs(model, N, s)) for s in DRAWS]
    bound = {k: ab.MARGIN * max(d[2][k] for d in drawn) for k in ("value", "head")}
    inputs, ref, _dist = drawn[0]
    dev = gl.device_inputs(inputs)
    act16, act32 = forward(m, model, dev, BF16), forward(m, model, dev, 0)
    var_amd.bind_convs(m, precision="bf16")
    with torch.no_grad():
        value, feats, _h, _ = m.base(gl.obs_of(model, dev), dev["hxs"], dev["masks"], infer=False)
        head = (m.dist.fc_mean if model == "arm" else m.dist.linear)(feats)
    torch.cuda.synchronize()
    ev = {"value": value.cpu(), "head": head.cpu()}
    for k in ("value", "head"):
        s = al.scale(ref[k])
        e_act, e_ev, gap = ab.rel(act16[k], ref[k]), ab.rel(ev[k], ref[k]), ab.rel(act16[k], ev[k], s)
        print(f"{model} {k:5s}: bound {bound[k]:.2e}  bf16 acting {e_act:.2e}  bf16 evaluation {e_ev:.2e}  between them {gap:.2e}"
              f"  (fp32 acting to bf16 evaluation {ab.rel(act32[k], ev[k], s):.2e})")
    gap16 = float((act16["head"] - ev["head"]).abs().max())
    gap32 = float((act32["head"] - ev["head"]).abs().max())
    # the sampled actions' importance ratio of the first evaluation, old log-probabilities from either acting forward
    g = torch.Generator().manual_seed(7)
    if model == "arm":
        action = act16["head"] + m.dist.logstd._bias.detach().cpu().view(1, -1).exp() * torch.randn(N, 2, generator=g)
    else:
        action = torch.multinomial(torch.softmax(act16["head"], -1), 1, generator=g)
    lp = {name: log_probs_host(model, P, h, action) for name, h in (("act16", act16["head"]), ("act32", act32["head"]), ("ev", ev["head"]))}
    r16 = float((torch.exp(lp["ev"] - lp["act16"]) - 1).abs().max())
    r32 = float((torch.exp(lp["ev"] - lp["act32"]) - 1).abs().max())
    print(f"{model}: max |d head| bf16 acting / bf16 evaluation {gap16:.3e}, fp32 acting / bf16 evaluation {gap32:.3e}; "
          f"max |ratio - 1| {r16:.3e} against {r32:.3e}")
    for k in ("value", "head"):
        s = al.scale(ref[k])
        assert ab.rel(act16[k], ref[k]) <= bound[k], (k, "acting")
        assert ab.rel(ev[k], ref[k]) <= bound[k], (k, "evaluation")
        assert ab.rel(act16[k], ev[k], s) <= 2 * bound[k], (k, "acting against evaluation")
    assert gap16 < gap32, (gap16, gap32)


def log_probs_host(model, P, head, action):
    if model == "arm":
        logstd = P["dist.logstd._bias"].view(1, -1)
        return (-0.5 * ((action - head) / logstd.exp()) ** 2 - logstd - 0.9189385332046727).sum(-1, keepdim=True)
    return torch.log_softmax(head, dim=-1).gather(1, action)

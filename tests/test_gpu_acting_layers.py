"""The acting forwards (var_armnet_forward, var_ithor_policy_forward: what every environment step and policy.capture(8) run),
pinned to float64 LAYER BY LAYER on every route.  One forward per case; then every buffer it left behind is read back
(var_debug_buffer's "arm_" / "ipol_" names) and each is checked alone: the float64 reference of tests/acting_layers_cpu.py
evaluated on the DEVICE'S OWN upstream buffers against the device's buffer -- the single layer, or the fused convolution + pool /
the run of Linear layers between two buffers that survive the call.  No error carries across checks, and no gate or tie rule is
needed: a forward max-pool's value does not depend on which of two equal entries wins.

Bound per check: MARGIN = 4 times the distance of torch's fp32 CPU kernels from float64 on those same inputs, relative to the
float64 array's largest magnitude (acting_layers_cpu.ORDER: the kernel's own accumulation order instead, where measured
necessary); the pool of the device's own map and rnn_hxs * masks are exact, bound 0.  value, head and rnn_hxs_out are also
compared end to end with the float64 chain at MARGIN times the end-to-end fp32 distance (cases b5p12, b8, b9: see E2E_ROWS).  tests/test_acting_layers_host.py shows
on the CPU that these checks fail for a dropped border column, band row or tap, a shifted pool window, a wrong row, a missing
addend, an ignored mask, swapped gates, a stale element and a NaN; DESIGN section 7 has the measured ratios.

Cases (the networks fix every spatial size; B, the plan, the inputs' form and the masks are free), each for both policies:
  b1     B 1, float image, mask 0: the smallest grid of every band kernel, the chain with one live row
  b8     B 8, u8 image of 4 channels (batch stride 4 x 96 x 96), mixed masks, two steps (the second from the first's state), checked
         after the second: every chain vector carries that launch's epoch in every row < B; get_value (no head) and a
         capture(8) replay leave the same bits in every buffer as the eager call
  b5p12  B 5 on a workspace planned for >= 12 (iTHOR: 5 actions): every maxB-based offset against every B-based stride
  b9     band convolutions + the per-layer MLP (the first batch past the chain): what survives the call, each from the nearest
         surviving buffer upstream
  b64    the last band batch; b65: the first gather-GEMM batch, with the un-pooled maps and exact pools.  The convolutions are
         compared on images 0, 31 and B - 1 (images are independent), the pools and the MLP on every row."""
import functools
import types

import pytest
import torch

from oracle.torch_oracle import armnet_seeded  # checker only
from tests import acting_layers_cpu as al

pytestmark = pytest.mark.gpu

MODELS = ("arm", "ipol")
CASES = {
    "b1": dict(B=1, u8=False, ch=3, masks=[0.0], seed=31),
    "b8": dict(B=8, u8=True, ch=4, seed=32, steps=2),
    "b5p12": dict(B=5, u8=True, ch=3, seed=33, plan=12, n_actions=5),
    "b9": dict(B=9, u8=False, ch=3, seed=34),
    "b64": dict(B=64, u8=True, ch=3, seed=35, images=[0, 31, 63]),
    "b65": dict(B=65, u8=True, ch=3, seed=36, images=[0, 31, 64]),
}
PREFIX = {"arm": "arm_", "ipol": "ipol_"}
MAP_SHAPE = {"arm": {"a1": (32, 96, 96), "a2": (32, 96, 96), "p1": (32, 48, 48), "a3": (64, 48, 48), "a4": (64, 48, 48),
                     "p2": (64, 24, 24), "a5": (128, 24, 24), "a6": (128, 24, 24), "p3": (128, 12, 12), "a7": (256, 5, 5), "a8": (1152,)},
             "ipol": {"a1": (32, 96, 96), "a2": (32, 96, 96), "p1": (32, 48, 48), "a3": (64, 48, 48), "p2": (64, 24, 24),
                      "a4": (64, 24, 24), "p3": (64, 12, 12), "a5": (128, 12, 12), "p4": (128, 6, 6), "a6": (1152,), "occf": (288,)}}
# the per-layer path's survivors: debug name, width (t0..t3: what their last writer left, csrc/actor_critic.h: layer_tail)
LAYER_BUFS = {"flat": ("flat_img", 256), "motor": ("motor", 256), "sound": ("sound", 256), "fusion": ("fusion", 256), "occ": ("occ", 256),
              "h0": ("h0", None), "gi": ("gi", None), "gh": ("gh", None), "all0": ("t2", 256), "all1": ("t3", 128), "c1": ("t1", 128),
              "a0": ("t0", 128)}
CHAIN_NAME = {"feats": "AFT"}
# End to end the yardstick is a maximum over B values (value is (B, 1)): asserted where every row of a batch of several is in it.
# At B = 1, and on the three compared rows of 64 / 65, it is one to three numbers -- torch's own fp32 at batch 65 sits at 0.87 of
# MARGIN x its three-row distance -- so there the figures are printed and the single-layer checks carry the case.
E2E_ROWS = (5, 8, 9)


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return m


class Box:
    shape = (2,)


class Discrete:
    def __init__(self, n):
        self.n = n


@functools.lru_cache(maxsize=None)
def policy(var_amd, model, n_actions=8):
    """(the policy on the device, its parameters on the host by state_dict key)"""
    if model == "arm":
        cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, robotStateDim=2)
        m = var_amd.ArmNetPolicy(None, Box(), config=cfg, base='arm_VAR', base_kwargs={
            'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 512, 'actionHiddenSize': 128})
        m.load_state_dict(armnet_seeded(453).state_dict())
    else:
        torch.manual_seed(977)
        m = var_amd.IthorNetPolicy(None, Discrete(n_actions), config=types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3),
                                   base='ai2thor_VAR', base_kwargs={'recurrent': True, 'recurrentInputSize': 128,
                                                                    'recurrentSize': 1024, 'actionHiddenSize': 128})
    P = {k: v.detach().clone().float() for k, v in m.state_dict().items()}
    return m.to("cuda"), P


def obs_of(model, dev):
    obs = {'image': dev["image"], 'image_feat': dev["image_feat"], 'goal_sound_feat': dev["goal"]}
    obs.update({'robot_pose': dev["robot_pose"]} if model == "arm" else {'occupancy': dev["occupancy"]})
    return obs


def forward(m, model, dev, head=True):
    """One C forward on device tensors as they are (a 4-channel image keeps its batch stride); outputs pre-filled with NaN."""
    from var_amd._lib import Context
    c = Context.get(0)
    B, H = dev["image"].shape[0], m.recurrent_hidden_state_size
    m._ensure_plan(c, B)
    out = lambda n: torch.full((B, n), float("nan"), device="cuda")      # noqa: E731
    value, feats, head_out, hout = out(1), out(128), out(m._n_head) if head else None, out(H)
    m._launch_forward(c, obs_of(model, dev), dev["hxs"], dev["masks"], value, feats, head_out, hout)
    torch.cuda.synchronize()
    got = {"value": value, "feats": feats, "hout": hout}
    if head:
        got["head"] = head_out
    return got


def read_back(model, B, H, got, head=True):
    """Every buffer the forward of B rows left behind, on the host under acting_layers_cpu's names; + 'tags' {vector: (B, width)
    int32}, 'epoch' (of the chain launch that ran) for B <= 8."""
    from var_amd._lib import Context
    ctx, pre = Context.get(0), PREFIX[model]
    b = {k: v.cpu() for k, v in got.items()}
    for k in al.survivors(model, B, head):
        if k in MAP_SHAPE[model]:
            sh = (B,) + MAP_SHAPE[model][k]
            n = 1
            for s in sh:
                n *= s
            b[k] = ctx.debug_buffer(pre + k, n).view(sh).cpu()
        elif B > al.CHAIN_ROWS and k in LAYER_BUFS:
            name, w = LAYER_BUFS[k]
            w = w or (H if k == "h0" else 3 * H)
            b[k] = ctx.debug_buffer(pre + name, B * w).view(B, w).cpu()
    if B <= al.CHAIN_ROWS:
        b["tags"] = {}
        for k in al.survivors(model, B, head):
            if k in b and k != "feats":
                continue
            raw = ctx.debug_buffer(pre + CHAIN_NAME.get(k, k.upper())).view(torch.int32).view(al.CHAIN_ROWS, -1, 2).cpu()
            vec = raw[:B, :, 0].contiguous().view(torch.float32)
            if k == "feats":                                          # the plain copy the caller gets is the handed-over vector
                assert torch.equal(vec, b[k])
            b[k], b["tags"][k] = vec, raw[:B, :, 1].contiguous()
        sync = ctx.debug_buffer(pre + "sync").view(torch.int32).cpu()
        b["epoch"] = int(sync[3]) - 1
    elif model == "ipol":
        assert torch.equal(ctx.debug_buffer(pre + "h1", B * H).view(B, H).cpu(), b["hout"])
    return b


def device_inputs(inputs):
    return {k: v.cuda().contiguous() for k, v in inputs.items()}


def run_case(var_amd, model, name):
    """(policy, parameters, host and device inputs of the checked step, every buffer it left)"""
    from var_amd._lib import Context
    spec = CASES[name]
    m, P = policy(var_amd, model, spec.get("n_actions", 8))
    ctx, B, H = Context.get(0), spec["B"], m.recurrent_hidden_state_size
    if "plan" in spec:
        m._call(ctx, "plan", spec["plan"])
        m._plan = max(m._plan, spec["plan"])
    inputs = al.random_inputs(model, B, spec["seed"], spec["u8"], spec["ch"], spec.get("masks"))
    assert inputs["image"].stride(0) == spec["ch"] * 96 * 96
    dev = device_inputs(inputs)
    got = forward(m, model, dev)
    for step in range(1, spec.get("steps", 1)):
        inputs = dict(inputs, hxs=got["hout"].cpu(), masks=torch.tensor([[float(r % 4 != step)] for r in range(B)]))
        dev = device_inputs(inputs)
        got = forward(m, model, dev)
    if "plan" in spec:
        assert ctx.debug_buffer_length(PREFIX[model] + "flat_img") // 256 >= spec["plan"] > B
    return m, P, inputs, dev, read_back(model, B, H, got)


@functools.lru_cache(maxsize=None)
def acting_step(var_amd, model):
    """Case b8, kept for the tests that compare other calls with it (the large cases are not kept)."""
    return run_case(var_amd, model, "b8")


@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("model", MODELS)
def test_every_layer_against_float64(var_amd, model, name):
    spec = CASES[name]
    m, P, inputs, _dev, b = acting_step(var_amd, model) if name == "b8" else run_case(var_amd, model, name)
    B, images = spec["B"], spec.get("images")
    keep = al.survivors(model, B)
    env = dict(inputs, **{k: b[k] for k in keep})
    tag = f"{model} {name}"
    with torch.no_grad():
        res = al.check_layers(model, env, P, keep, images=images, order=al.order_for(model, B), log=lambda s: print(f"{tag}: {s}"))
        sub = (lambda t: t[images]) if images else (lambda t: t)
        e2e = al.end_to_end(model, P, {k: sub(v) for k, v in inputs.items()}, {k: sub(b[k]) for k in al.OUTPUTS})
    assert list(res) == keep and len(e2e) == 3
    for k, (err, dist, q) in e2e.items():
        print(f"{tag}: end to end {k:6s} err {err:.2e} dist {dist:.2e} ratio {q:.3f}")
    bad = [(k, r) for k, r in res.items() if not r[3] <= 1]                    # (not "any ratio > 1": a NaN must not pass)
    if B in E2E_ROWS:
        bad += [("end to end " + k, r) for k, r in e2e.items() if not r[2] <= 1]
    inexact = [k for k in keep if (k == "h0" or (k.startswith("p") and B > al.BAND_MAX_B)) and res[k][2] != 0]
    assert not inexact, inexact                                                # routing and selection: distance 0, bound 0
    assert not bad, bad
    assert m.chain_status() == 0


@pytest.mark.parametrize("model", MODELS)
def test_second_step_reads_nothing_of_the_first_and_get_value_leaves_the_same_bits(var_amd, model):
    m, _P, _inputs, dev, b = acting_step(var_amd, model)
    B, H = 8, m.recurrent_hidden_state_size
    vectors = [k for k in al.survivors(model, B) if k not in al.MAPS[model] and k not in ("value", "head", "hout")]
    assert sorted(b["tags"]) == sorted(vectors) and len(vectors) == (21 if model == "arm" else 22)
    assert b["epoch"] >= 2
    stale = [k for k, t in b["tags"].items() if not bool((t == b["epoch"]).all())]
    assert not stale, stale
    again = read_back(model, B, H, forward(m, model, dev, head=False), head=False)
    assert set(again) == set(b) - {"head"}
    diff = [k for k in again if torch.is_tensor(again[k]) and not torch.equal(again[k], b[k])]
    assert not diff, diff
    stale = [k for k, t in again["tags"].items() if not bool((t == again["epoch"]).all())]
    assert not stale, stale


@pytest.mark.parametrize("model", MODELS)
def test_a_captured_replay_leaves_the_eager_calls_bits_in_every_buffer(var_amd, model):
    m, _P = policy(var_amd, model)
    B, H = 8, m.recurrent_hidden_state_size
    inputs = al.random_inputs(model, B, 41, u8=True, channels=3)
    dev = device_inputs(inputs)
    eager = read_back(model, B, H, forward(m, model, dev))
    step = m.capture(B, deterministic=True, image_dtype=torch.uint8)
    step.reset(dev["hxs"])
    value, _action, _logp, hout = step(obs_of(model, dev), dev["masks"])
    torch.cuda.synchronize()
    replay = read_back(model, B, H, {"value": value, "feats": step.actor_features, "head": step.head, "hout": hout})
    assert set(replay) == set(eager) and replay["epoch"] > eager["epoch"]
    diff = [k for k in eager if torch.is_tensor(eager[k]) and not torch.equal(eager[k], replay[k])]
    assert not diff, diff
    stale = [k for k, t in replay["tags"].items() if not bool((t == replay["epoch"]).all())]
    assert not stale, stale

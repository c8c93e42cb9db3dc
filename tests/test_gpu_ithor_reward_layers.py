"""The frozen iTHOR encoder's reward step (var_ithor_reward_plan / _pack / _step: what every environment step of the RL stage
runs, and the signal PPO trains on), pinned to float64 LAYER BY LAYER on every route.  Each case runs one goal step and one
image-only step through the C entry point; after each, every buffer the step left behind is read back (var_debug_buffer's
"irew_" names) and each row of tests/ithor_reward_layers_cpu.py's table is checked alone: the float64 reference evaluated on the
DEVICE'S OWN upstream buffers against the device's buffer.  No error carries across rows.

Bound per row: MARGIN = 4 times the distance of torch's fp32 CPU kernels from float64 on those same inputs, relative to the
float64 array's largest magnitude (ithor_reward_layers_cpu.ORDER: the kernel's own accumulation order instead, where measured
necessary); the snapshot and what an image-only step leaves alone are exact.  tests/test_ithor_reward_layers_host.py shows on the
CPU which faults these rows catch; DESIGN section 7 has the measured ratios.

Cases (the network fixes every spatial size; B, the plan and the inputs' form are free):
  b1   B 1, float image, the clip all-zero: the smallest grids, the tail with one live row
  b8   B 8, u8 image of 4 channels (batch stride 4 x 96 x 96), clips cut at several lengths
  b5   B 5 under a plan of at least 12: every maxB-based offset against every B-based stride
  b16  the last batch of the fused GRU step; b17: the first of the split-K product + gate pair
  b64  the band kernels' and the plan's limit.  At 17 and 64 the convolutions are compared on the first, a middle and the
       last image / clip (they are independent), every other row on all rows."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _ithor_reward_inputs as rin
from tests import ithor_reward_layers_cpu as rl

pytestmark = pytest.mark.gpu

CASES = {
    "b1": dict(B=1, u8=False, ch=3, seed=51, silent=[0]),
    "b8": dict(B=8, u8=True, ch=4, seed=52),
    "b5": dict(B=5, u8=True, ch=3, seed=53, plan=12),
    "b16": dict(B=16, u8=True, ch=3, seed=54, silent=[15]),
    "b17": dict(B=17, u8=True, ch=3, seed=55, silent=[3], images=[0, 16]),
    "b64": dict(B=64, u8=True, ch=3, seed=56, images=[0, 31, 63]),
}
SHAPES = {"a1": (32, 96, 96), "p1": (32, 48, 48), "p2": (64, 24, 24), "p3": (64, 12, 12), "p4": (128, 6, 6), "a6": (1152,), "hid": (128,),
          "s1": (64, 300, 20), "s2": (64, 150, 13), "s3": (73, 448), "hs1": (128,), "hs2": (64,), "graw": (3,)}
ERR_ARG, ERR_PLAN = -1, -3
NAN = float("nan")


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return m


@functools.lru_cache(maxsize=None)
def encoder(var_amd):
    """(the model on the device, its parameters on the host by state_dict key, its arena)"""
    import types
    checker = rin.spread_checker()
    m = var_amd.IthorVARPretextNet(types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 600, 40), representationDim=3))
    m.load_state_dict(checker.state_dict())
    m = m.to("cuda").eval()
    P = {k: v.detach().clone().float() for k, v in checker.state_dict().items()}
    flat = m.flat_parameters()
    assert torch.equal(flat.detach().cpu(), rl.arena_of(P))
    return m, P, flat


def context():
    from var_amd._lib import Context
    return Context.get(0)


def plan_and_pack(flat, B):
    from var_amd._lib import current_stream_handle, ptr
    c = context()
    c.check(c.lib.var_ithor_reward_plan(c.handle, int(B), 96), "var_ithor_reward_plan")
    c.check(c.lib.var_ithor_reward_pack(c.handle, current_stream_handle(), ptr(flat)), "var_ithor_reward_pack")
    maxB = c.debug_buffer_length("irew_hid") // 128                # (the context's reward plan only grows)
    assert maxB >= B
    return maxB


def step(flat, image, goal, B, goal_feat=None):
    """var_ithor_reward_step on the current stream; outputs pre-filled with NaN (an image-only step is given the goal step's
    goal_feat, which it reads).  Returns (image_feat, goal_feat, reward) on the device."""
    from var_amd._lib import current_stream_handle, ptr
    c = context()
    out = lambda *s: torch.full(s, NAN, device="cuda")      # noqa: E731
    image_feat, reward = out(B, 3), out(B)
    goal_feat = out(B, 3) if goal_feat is None else goal_feat.clone()
    c.check(c.lib.var_ithor_reward_step(c.handle, current_stream_handle(), ptr(flat), ptr(image), int(image.dtype == torch.uint8),
                                        image.stride(0), ptr(goal), B, ptr(image_feat), ptr(goal_feat), ptr(reward)),
            "var_ithor_reward_step")
    torch.cuda.synchronize()
    return image_feat, goal_feat, reward


def snapshot(B, maxB):
    """Every "irew_" buffer on the device, cut to what a step of B rows fills (strides as csrc/ithor_reward.hip: goal_branch)."""
    c = context()
    b = {k: c.debug_buffer("irew_" + k, B * int(np.prod(sh))).view((B,) + sh) for k, sh in SHAPES.items()}
    b["gi"] = c.debug_buffer("irew_gi", 2 * B * 73 * 1536).view(2, B, 73, 1536)
    b["gh"] = c.debug_buffer("irew_gh", rl.REC_SPLIT * 2 * B * 1536).view(rl.REC_SPLIT, 2, B, 1536)
    b["h72"] = c.debug_buffer("irew_hb", B * 1024).view(B, 1024)
    b["h73"] = c.debug_buffer("irew_hb", B * 1024, offset=maxB * 1024).view(B, 1024)
    b["frozen"] = c.debug_buffer("irew_frozen")
    assert c.debug_buffer_length("irew_hb") == 2 * maxB * 1024 and c.debug_buffer_length("irew_gi") == 2 * maxB * 73 * 1536
    return b


def poke(name, src, offset=0):
    """src (a device tensor of floats) into the named buffer from `offset`, through the pointer var_debug_buffer returns."""
    from var_amd._lib import _i, _l, _vp
    c = context()
    p, n = _vp(), _l()
    c.check(c.lib.var_debug_buffer(c.handle, name.encode(), ctypes.byref(p), ctypes.byref(n)), "var_debug_buffer")
    assert src.is_cuda and src.dtype == torch.float32 and src.is_contiguous() and 0 <= offset and offset + src.numel() <= n.value
    torch.cuda.synchronize()
    rt = ctypes.CDLL("libamdhip64.so")
    rt.hipMemcpy.argtypes = [_vp, _vp, ctypes.c_size_t, _i]
    assert rt.hipMemcpy(p.value + 4 * offset, src.data_ptr(), src.numel() * 4, 3) == 0      # hipMemcpyDeviceToDevice


def case_inputs(name, seed_shift=0):
    """(image, goal) on the device as the case wants them."""
    spec = CASES[name]
    B = spec["B"]
    img, snd = rin.spread_inputs(B, spec["seed"] + seed_shift)
    for i in spec.get("silent", []):
        snd[i] = 0.0
    image = torch.from_numpy(img)
    if spec["ch"] == 4:
        image = torch.cat([image, torch.full((B, 1, 96, 96), 201, dtype=torch.uint8)], 1)      # a plane the kernels must not read
    if not spec["u8"]:
        image = image.float() / 255
    image = image.cuda().contiguous()
    assert image.stride(0) == spec["ch"] * 96 * 96
    return image, torch.from_numpy(snd).cuda()


def run_checks(tag, env, P, route, goal, images, B):
    with torch.no_grad():
        res = rl.check_layers(env, P, route, goal=goal, images=images, order=rl.order_for(route), log=lambda s: print(f"{tag}: {s}"))
    assert list(res) == [r.name for r in rl.rows(route, goal)]
    bad = [(k, r) for k, r in res.items() if not r[2] <= 1]                     # (not "any ratio > 1": a NaN must not pass)
    assert res["frozen"][0] == 0 and res["frozen"][1] == 0
    assert not bad, bad


@pytest.mark.parametrize("name", list(CASES))
def test_every_row_against_float64(var_amd, name):
    spec = CASES[name]
    _m, P, flat = encoder(var_amd)
    B, images, route = spec["B"], spec.get("images"), rl.route_of(spec["B"])
    maxB = plan_and_pack(flat, spec.get("plan", B))
    assert maxB >= spec.get("plan", B)
    image, goal = case_inputs(name)
    outs = step(flat, image, goal, B)
    dev = snapshot(B, maxB)
    env = {k: v.cpu() for k, v in dev.items() if k != "gh" or route == "split"}
    env.update(image=image.cpu(), goal=goal.cpu(), arena=flat.detach().cpu(), **{k: v.cpu() for k, v in zip(rl.OUTPUTS, outs)})
    run_checks(f"{name} goal step", env, P, route, True, images, B)
    # the image-only step: other images, the cached goal
    image2, _ = case_inputs(name, seed_shift=20)
    outs2 = step(flat, image2, None, B, goal_feat=outs[1])
    dev2 = snapshot(B, maxB)
    changed = [k for k in rl.SOUND_SIDE if not torch.equal(dev2[k], dev[k])]
    assert not changed, changed                                                  # bit for bit: bound 0
    assert torch.equal(outs2[1], outs[1]), "the cached goal embedding changed in an image-only step"
    env2 = {k: dev2[k].cpu() for k in rl.IMAGE_SIDE if k in dev2}
    env2.update(image=image2.cpu(), arena=env["arena"], frozen=dev2["frozen"].cpu(), **{k: v.cpu() for k, v in zip(rl.OUTPUTS, outs2)})
    assert not torch.equal(env2["a1"], env["a1"])
    run_checks(f"{name} image-only step", env2, P, route, False, images, B)


@pytest.mark.parametrize("name", ["b8", "b17"])
def test_a_goal_step_reads_nothing_of_the_state_slots_or_the_slabs(var_amd, name):
    """Both hb slots and gh full of NaN before the goal step: the outputs and h73 are finite and equal, bit for bit, those of the
    same step from zeroed slots (step 0 reads no state and adds no slab)."""
    _m, _P, flat = encoder(var_amd)
    B = CASES[name]["B"]
    maxB = plan_and_pack(flat, B)
    image, goal = case_inputs(name)
    c = context()
    got = []
    for fill in (NAN, 0.0):
        poke("irew_hb", torch.full((c.debug_buffer_length("irew_hb"),), fill, device="cuda"))
        poke("irew_gh", torch.full((c.debug_buffer_length("irew_gh"),), fill, device="cuda"))
        outs = step(flat, image, goal, B)
        got.append(list(outs) + [snapshot(B, maxB)[k] for k in ("h72", "h73", "hs1", "graw")])
    for a, z in zip(*got):
        assert bool(torch.isfinite(a).all()), "a NaN of the state slots reached the step's results"
        assert torch.equal(a, z)


def test_normalisation_floor_gives_zero_rows(var_amd):
    """A head whose last Linear is zero has raw output 0: x / max(|x|, 1e-12) is exactly 0 (F.normalize's result), not NaN."""
    _m, P, flat = encoder(var_amd)
    B = 8
    plan_and_pack(flat, B)
    image, goal = case_inputs("b8")
    offset, o = {}, 0
    for k, v in P.items():
        offset[k] = (o, o + v.numel())
        o += v.numel()
    try:
        for head, zero in (("imgTriplet.2", (0, 2)), ("soundTriplet.4", (1, 2))):
            arena = flat.detach().clone()
            for k in (head + ".weight", head + ".bias"):
                arena[offset[k][0]:offset[k][1]] = 0
            plan_and_pack(arena, B)
            outs = step(arena, image, goal, B)
            for i, t in enumerate(outs):
                assert bool(torch.isfinite(t).all()), (head, rl.OUTPUTS[i])
                if i in zero:
                    assert bool((t == 0).all()), (head, rl.OUTPUTS[i], t)
                else:
                    assert float(t.abs().max()) > 0.1
            if head == "imgTriplet.2":                      # and the image-only step's tail alike
                outs2 = step(arena, image, None, B, goal_feat=outs[1])
                assert bool((outs2[0] == 0).all()) and bool((outs2[2] == 0).all()) and torch.equal(outs2[1], outs[1])
    finally:
        plan_and_pack(flat, B)


def test_snapshot_keeps_the_packed_bits_until_the_next_pack(var_amd):
    _m, _P, flat = encoder(var_amd)
    B = 8
    maxB = plan_and_pack(flat, B)
    image, goal = case_inputs("b8")
    c = context()
    before = flat.detach().clone()
    outs = step(flat, image, goal, B)
    assert torch.equal(c.debug_buffer("irew_frozen"), before)
    try:
        with torch.no_grad():
            flat[:64] += 1.0                                 # conv 1's first filters, in place
        torch.cuda.synchronize()
        assert torch.equal(c.debug_buffer("irew_frozen"), before) and not torch.equal(flat.detach(), before)
        again = step(flat, image, goal, B)
        assert all(torch.equal(a, o) for a, o in zip(again, outs)), "a step followed the arena, not the snapshot"
        plan_and_pack(flat, B)
        assert torch.equal(c.debug_buffer("irew_frozen"), flat.detach())
        moved = step(flat, image, goal, B)
        assert not torch.equal(moved[0], outs[0])
    finally:
        with torch.no_grad():
            flat.copy_(before)
        plan_and_pack(flat, B)
    assert torch.equal(snapshot(B, maxB)["frozen"], before)


def test_a_captured_replay_leaves_the_eager_calls_bits_in_every_buffer(var_amd):
    m, _P, flat = encoder(var_amd)
    B = 8
    image, goal = case_inputs("b5")                          # (3 channels, contiguous)
    image, goal = torch.cat([image, image[:3]]), torch.cat([goal, goal[:3]])
    r = var_amd.IntrinsicReward(m).capture(B)
    maxB = context().debug_buffer_length("irew_hid") // 128
    outs = [t.clone() for t in r.step(image, goal)]
    torch.cuda.synchronize()
    replay = snapshot(B, maxB)
    c = context()

    def spoil(names):      # every whole buffer NaN, so that equal bits afterwards are the eager call's own
        for k in names:
            poke("irew_" + k, torch.full((c.debug_buffer_length("irew_" + k),), NAN, device="cuda"))

    # (gh is left alone: at 8 clips the fused GRU step never writes it, so both calls must leave its bits as they are)
    spoil(("a1", "p1", "p2", "p3", "p4", "a6", "hid", "s1", "s2", "s3", "gi", "hb", "hs1", "hs2", "graw"))
    eager_outs = step(flat, image, goal, B)
    eager = snapshot(B, maxB)
    assert all(torch.equal(a, o) for a, o in zip(eager_outs, outs))
    assert all(bool(torch.isfinite(v).all()) for k, v in eager.items() if k != "gh")
    diff = [k for k in eager if not torch.equal(eager[k].view(torch.int32), replay[k].view(torch.int32))]
    assert not diff, diff
    outs2 = [t.clone() for t in r.step(case_inputs("b8", 20)[0][:, :3].contiguous())]
    torch.cuda.synchronize()
    replay2 = snapshot(B, maxB)
    spoil(("a1", "p1", "p2", "p3", "p4", "a6", "hid"))       # what an image-only step writes
    eager_outs2 = step(flat, case_inputs("b8", 20)[0][:, :3].contiguous(), None, B, goal_feat=outs[1])
    eager2 = snapshot(B, maxB)
    assert all(torch.equal(a, o) for a, o in zip(eager_outs2, outs2))
    assert all(bool(torch.isfinite(eager2[k]).all()) for k in rl.IMAGE_SIDE[:-1])
    diff = [k for k in eager2 if not torch.equal(eager2[k].view(torch.int32), replay2[k].view(torch.int32))]
    assert not diff, diff


def test_irew_names_are_refused_without_a_plan_and_when_unknown(var_amd):
    from var_amd._lib import Context, _l, _vp
    _m, _P, flat = encoder(var_amd)
    plan_and_pack(flat, 1)
    p, n = _vp(), _l()
    c = context()
    for name in (b"irew_", b"irew_a2", b"irew_p5", b"irew_hb1", b"irew_HID"):
        assert c.lib.var_debug_buffer(c.handle, name, ctypes.byref(p), ctypes.byref(n)) == ERR_ARG, name
        assert not p.value and n.value == 0
    assert b"reward buffer" in c.lib.var_last_error(c.handle)
    fresh = Context(0)                                       # a context of its own: nothing planned yet
    try:
        assert fresh.lib.var_debug_buffer(fresh.handle, b"irew_hid", ctypes.byref(p), ctypes.byref(n)) == ERR_PLAN
        assert b"var_ithor_reward_plan" in fresh.lib.var_last_error(fresh.handle)
    finally:
        fresh.lib.var_destroy(fresh.handle)
        fresh.handle = None

"""GPU checks of the env wrapper's device step (csrc/env_step.hip: var_reward_norm_step, var_rollout_move_at; var_amd.collect:
DeviceReturnNormalizer, CollectStep).

Bounds.  There are none: every comparison is bit for bit.  The normaliser's float64 state (ret, mean, var, count) contains only
additions, multiplications and divisions, each rounded once in the host's grouping, summed in numpy's order (the restatement of
tests/env_step_cpu.py, pinned to var_amd.ReturnNormalizer and to the reference's fixture by tests/test_env_step_host.py); the
float32 reward is float32 of the host's float64 quotient, whose division and sqrt are IEEE operations, correctly rounded in
float64 on the device.  The copies move bytes.  End to end both legs run the same kernels on the same bits."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import env_step_cpu as es

pytestmark = pytest.mark.gpu

ERR_ARG = -1
CANARY = 0xA5


class Discrete:
    def __init__(self, n=8):
        self.n = n


class Box:
    def __init__(self, n=2):
        self.shape = (n,)


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


def p(t):
    return None if t is None else t.data_ptr()


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


@functools.lru_cache(maxsize=None)
def seq(n):
    return es.sequence(n)


def run_device(var_amd, n, inputs, num_steps=1, **kw):
    """A sequence through DeviceReturnNormalizer, every output logged on the device and read once."""
    dot, env, done, bad = inputs
    norm = var_amd.DeviceReturnNormalizer(n, num_steps=num_steps, **kw)
    steps = env.shape[0]
    d_dot = None if dot is None else dev(dot)
    d_env, d_done, d_bad = dev(env), dev(done.astype(np.uint8)), None if bad is None else dev(bad.astype(np.uint8))
    log = {k: [] for k in ("reward", "masks", "bad_masks", "orig", "ret", "rms", "episode", "slot")}
    for t in range(steps):
        r = norm(None if d_dot is None else d_dot[t], d_env[t], d_done[t], None if d_bad is None else d_bad[t])
        assert r is norm.reward
        for k, v in (("reward", norm.reward), ("masks", norm.masks), ("bad_masks", norm.bad_masks), ("orig", norm.orig_reward),
                     ("ret", norm.ret), ("rms", norm.rms), ("episode", norm.episode), ("slot", norm.slot)):
            log[k].append(v.clone())
    return norm, {k: host(torch.stack(v)) for k, v in log.items()}


# ---- var_reward_norm_step ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", es.NS)
def test_norm_step_equals_the_host_normalizer_bit_for_bit(var_amd, n):
    want = es.run_host_normalizer(var_amd, n, seq(n))
    rest = es.run_restatement(n, seq(n), num_steps=3)
    norm, got = run_device(var_amd, n, seq(n), num_steps=3)
    assert np.array_equal(bits64(got["ret"]), bits64(want["ret"]))
    assert np.array_equal(bits64(got["rms"]), bits64(want["rms"]))
    assert np.array_equal(bits32(got["reward"][..., 0]), bits32(want["out64"].astype(np.float32)))
    dot, env, done, bad = seq(n)
    assert np.array_equal(got["masks"][..., 0], 1.0 - done) and np.array_equal(got["bad_masks"][..., 0], 1.0 - bad)
    assert np.array_equal(bits64(got["orig"]), bits64(dot.astype(np.float64) + env))
    assert np.array_equal(bits64(got["episode"][-1]), bits64(rest["episode"]))
    assert np.array_equal(got["slot"], np.array([[(t + 1) % 3, t % 3] for t in range(es.STEPS)], np.int32))
    mean, var, count, ret = norm.state()
    assert (mean, var, count) == tuple(want["rms"][-1]) and np.array_equal(ret, want["ret"][-1])
    h = norm.to_host()                                           # a run resumes on the host where the device left it ...
    back = var_amd.DeviceReturnNormalizer(n).load(h)             # ... and the other way round
    a = h(dot[0].astype(np.float64) + env[0], done[0])
    b = back(dev(dot[0]), dev(env[0]), dev(done[0]))
    assert np.array_equal(bits32(host(b)[:, 0]), bits32(a.astype(np.float32))) and np.array_equal(bits64(back.state()[3]), bits64(h.ret))


def test_norm_step_reproduces_the_reference_fixture(var_amd, golden_dir):
    fx = dict(np.load(os.path.join(golden_dir, "reward_norm.npz")))
    n = fx["rews"].shape[1]
    for clip, key in ((10.0, "out"), (1.5, "out_clip15")):
        norm, got = run_device(var_amd, n, (None, fx["rews"], fx["news"], None), cliprew=clip)
        assert np.array_equal(bits32(got["reward"][..., 0]), bits32(fx[key].astype(np.float32))), key
        assert tuple(got["rms"][-1]) == (float(fx["mean"]), float(fx["var"]), float(fx["count"]))
        assert (got["bad_masks"] == 1).all()
    assert np.abs(got["reward"]).max() == 1.5


def test_norm_step_without_normalisation_across_a_slot_wrap(var_amd):
    n, T = 9, 3
    dot, env, done, bad = (a[:8] for a in seq(n))
    rest = es.NormStep(n, normalise=False, num_steps=T)
    norm, got = run_device(var_amd, n, (dot, env, done, bad), num_steps=T, normalize=False)
    for t in range(8):
        r32, masks, bm, orig, _ = rest(dot[t], env[t], done[t], bad[t])
        assert np.array_equal(bits32(got["reward"][t]), bits32(r32)) and np.array_equal(got["masks"][t], masks)
        assert np.array_equal(got["bad_masks"][t], bm) and np.array_equal(bits64(got["orig"][t]), bits64(orig))
        assert np.array_equal(bits64(got["ret"][t]), bits64(rest.ret)) and np.array_equal(bits64(got["episode"][t]), bits64(rest.episode))
        assert np.array_equal(got["slot"][t], rest.slot) and tuple(got["slot"][t]) == ((t + 1) % T, t % T)
        assert np.array_equal(got["rms"][t], [0.0, 1.0, 1e-4])
    assert got["episode"][-1][2].sum() == done.sum() > 0


def norm_args(n, fill=7.0):
    f64 = lambda k: torch.full((k,), fill, dtype=torch.float64, device="cuda")   # noqa: E731
    f32 = lambda: torch.full((n, 1), fill, device="cuda")                        # noqa: E731
    return dict(dot=torch.zeros(n, device="cuda"), env=torch.zeros(n, dtype=torch.float64, device="cuda"),
                done=torch.zeros(n, dtype=torch.uint8, device="cuda"), bad=torch.zeros(n, dtype=torch.uint8, device="cuda"),
                ret=f64(n), rms=f64(3), episode=f64(3 * n), slot=torch.full((2,), 7, dtype=torch.int32, device="cuda"),
                reward=f32(), masks=f32(), bad_masks=f32(), orig=f64(n))


def call_norm(ctx, a, n, num_steps=3, normalise=1):
    return ctx.lib.var_reward_norm_step(ctx.handle, None, p(a["dot"]), p(a["env"]), p(a["done"]), p(a["bad"]), n, 0.99, 10.0, 1e-8,
                                        normalise, num_steps, p(a["ret"]), p(a["rms"]), p(a["episode"]), p(a["slot"]), p(a["reward"]),
                                        p(a["masks"]), p(a["bad_masks"]), p(a["orig"]))


def test_norm_step_refuses_bad_arguments_and_writes_nothing(ctx):
    n = 8
    a = norm_args(128)
    outs = ("ret", "rms", "episode", "slot", "reward", "masks", "bad_masks", "orig")
    cases = [dict(n=0), dict(n=129), dict(num_steps=0), dict(null="env"), dict(null="done"), dict(null="ret"), dict(null="rms"),
             dict(null="episode"), dict(null="slot"), dict(null="reward"), dict(null="masks"), dict(null="bad_masks"), dict(null="orig"),
             dict(alias=("masks", "reward")), dict(alias=("orig", "ret")), dict(alias=("env", "ret"))]
    for case in cases:
        b = dict(a)
        if "null" in case:
            b[case["null"]] = None
        if "alias" in case:
            b[case["alias"][0]] = b[case["alias"][1]]
        rc = call_norm(ctx, b, case.get("n", n), case.get("num_steps", 3))
        assert rc == ERR_ARG, case
        assert ctx.lib.var_last_error(ctx.handle)
    torch.cuda.synchronize()
    for k in outs:
        assert (a[k] == 7).all(), k
    assert call_norm(ctx, dict(a, dot=None, bad=None), n) == 0   # (the two pointers that may be NULL)
    torch.cuda.synchronize()
    assert (a["reward"][:n] == 0).all() and (a["reward"][n:] == 7).all() and (a["bad_masks"][:n] == 1).all()
    assert a["slot"].tolist() == [8 % 3, 7]


# ---- var_rollout_move_at ----------------------------------------------------------------------------------------------------
ROWS = {"wide": ((64,), torch.float32), "scalar": ((1,), torch.float32), "action": ((1,), torch.int64), "image": ((3, 5, 5), torch.uint8),
        "big_image": ((3, 37, 37), torch.uint8)}
ADD = {"wide": 1, "scalar": 0, "action": 0, "image": 1, "big_image": 1}


def move_parts(N, T, seed=0):
    g = torch.Generator().manual_seed(seed)
    src, store = {}, {}
    for k, (shape, dt) in ROWS.items():
        nbytes = N * int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
        src[k] = torch.randint(0, 256, (nbytes,), dtype=torch.uint8, generator=g).cuda().view(dt).view(N, *shape)
    for k, (shape, dt) in ROWS.items():
        nbytes = (T + ADD[k]) * N * int(np.prod(shape)) * torch.empty((), dtype=dt).element_size()
        store[k] = torch.full((nbytes,), CANARY, dtype=torch.uint8, device="cuda").view(dt).view(T + ADD[k], N, *shape)
    return src, store


def at_table(var_amd, src, store, N, names=None, stride0=()):
    from var_amd._lib import MoveAtSeg, MoveSeg
    segs = []
    for k in names or ROWS:
        rb = src[k].numel() // N * src[k].element_size()
        if k in stride0:
            segs.append(MoveAtSeg(MoveSeg(p(src[k]), p(store[k][1]), rb, 1, 0, 0, rb, rb), 0, 5, 1))
        else:
            segs.append(MoveAtSeg(MoveSeg(p(src[k]), p(store[k]), rb, 1, 0, 0, rb, rb), N * rb, ADD[k], store[k].shape[0]))
    return (MoveAtSeg * len(segs))(*segs)


def move_to(ctx, src, store, N, slot, names=None):
    """The reference: var_rollout_move to host-computed addresses, segments whose slot is outside the store left out."""
    from var_amd._lib import MoveSeg
    segs = []
    for k in names or ROWS:
        s = slot + ADD[k]
        if 0 <= s < store[k].shape[0]:
            rb = src[k].numel() // N * src[k].element_size()
            segs.append(MoveSeg(p(src[k]), p(store[k][s]), rb, 1, 0, 0, rb, rb))
    if segs:
        assert ctx.lib.var_rollout_move(ctx.handle, None, (MoveSeg * len(segs))(*segs), len(segs), None, N, N) == 0


def raw(t):
    return host(t.contiguous().view(-1).view(torch.uint8))


@pytest.mark.parametrize("slot", [0, 2, 3, -1, -7])
def test_move_at_equals_move_to_host_addresses(var_amd, ctx, slot):
    """T = 3: slot words 0 and T - 1 (slot_add = 1 then reaches slot T); T and -7 select nothing anywhere; -1 only slot 0 of the
    slot_add = 1 stores.  Rows: 16-byte pieces, (N,1) f32, (N,1) int64, a 75-byte u8 image row, a u8 row of 257 pieces."""
    N, T = 5, 3
    src, got = move_parts(N, T)
    _, want = move_parts(N, T)
    word = dev(np.array([99, slot, 99], np.int32))
    rc = ctx.lib.var_rollout_move_at(ctx.handle, None, at_table(var_amd, src, got, N), len(ROWS), p(word) + 4, N)
    assert rc == 0, ctx.lib.var_last_error(ctx.handle)
    move_to(ctx, src, want, N, slot)
    written = 0
    for k in ROWS:
        assert np.array_equal(raw(got[k]), raw(want[k])), k
        written += int((raw(got[k]) != CANARY).any())
    assert written == {0: 5, 2: 5, 3: 0, -1: 3, -7: 0}[slot]
    if slot == 2:
        assert np.array_equal(raw(got["wide"][3]), raw(src["wide"])) and np.array_equal(raw(got["action"][2]), raw(src["action"]))
    assert word.tolist() == [99, slot, 99]


def test_move_at_with_slot_stride_zero_is_a_plain_copy(var_amd, ctx):
    N, T = 5, 3
    src, got = move_parts(N, T)
    word = dev(np.array([-40], np.int32))                       # not consulted by a stride-0 segment; outside for the others
    tab = at_table(var_amd, src, got, N, stride0=("wide", "image"))
    assert ctx.lib.var_rollout_move_at(ctx.handle, None, tab, len(ROWS), p(word), N) == 0
    torch.cuda.synchronize()
    for k in ROWS:
        if k in ("wide", "image"):
            assert np.array_equal(raw(got[k][1]), raw(src[k])) and (raw(got[k][0]) == CANARY).all() and (raw(got[k][2:]) == CANARY).all()
        else:
            assert (raw(got[k]) == CANARY).all(), k


def test_move_at_refuses_bad_arguments_and_writes_nothing(var_amd, ctx):
    from var_amd._lib import MoveAtSeg, MoveSeg
    N, T = 5, 3
    src, store = move_parts(N, T)
    word = dev(np.array([1], np.int32))
    good = at_table(var_amd, src, store, N)
    call = lambda tab, n, w=word, envs=N: ctx.lib.var_rollout_move_at(ctx.handle, None, tab, n, p(w), envs)   # noqa: E731
    assert call(good, 0) == ERR_ARG and call(None, 1) == ERR_ARG and call(good, len(ROWS), None) == ERR_ARG
    assert call(good, len(ROWS), word, 0) == ERR_ARG
    many = (MoveAtSeg * 17)(*([good[0]] * 17))
    assert call(many, 17) == ERR_ARG

    def one(k, **ch):
        rb = src[k].numel() // N * src[k].element_size()
        f = dict(src=p(src[k]), dst=p(store[k]), stride=N * rb, add=ADD[k], n_slots=store[k].shape[0], rb=rb)
        f.update(ch)
        return MoveAtSeg(MoveSeg(f["src"], f["dst"], f["rb"], 1, 0, 0, f["rb"], f["rb"]), f["stride"], f["add"], f["n_slots"])

    bad = {"two segments into one store (their slot ranges overlap)": [one("scalar"), one("scalar", add=1, n_slots=2)],
           "a later slot of the destination is the source": [one("wide", src=p(store["wide"][2]))],
           "no slots": [one("wide", n_slots=0)], "negative slot stride": [one("wide", stride=-16)],
           "slots that overlap each other": [one("wide", stride=16)], "stride 0 with several slots": [one("wide", stride=0)],
           "NULL source": [one("wide", src=None)], "empty rows": [one("wide", rb=0)],
           "the slot word inside a destination": [one("scalar")]}
    for why, segs in bad.items():
        w = word
        if why.startswith("the slot word"):
            w = store["scalar"].view(-1).view(torch.int32)[7:]
        assert call((MoveAtSeg * len(segs))(*segs), len(segs), w) == ERR_ARG, why
        assert ctx.lib.var_last_error(ctx.handle)
    torch.cuda.synchronize()
    for k in ROWS:
        assert (raw(store[k]) == CANARY).all(), k


# ---- CollectStep ------------------------------------------------------------------------------------------------------------
N_ENVS, T_STEPS, N_OBSERVE, GOAL_STEP, ALL_DONE = 8, 3, 8, 4, 6


@functools.lru_cache(maxsize=None)
def models(which):
    import var_amd
    torch.manual_seed(453)
    if which == "arm":
        enc = var_amd.VARPretextNet(types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 100, 40), representationDim=3))
        cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, robotStateDim=2, RLObsIgnore=[])
        pol = var_amd.ArmNetPolicy(None, Box(), config=cfg, base='arm_VAR', base_kwargs={
            'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 512, 'actionHiddenSize': 128})
        space = Box()
    else:
        enc = var_amd.IthorVARPretextNet(types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 600, 40), representationDim=3))
        cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, RLObsIgnore=[])
        pol = var_amd.IthorNetPolicy(None, Discrete(), config=cfg, base='ai2thor_VAR', base_kwargs={
            'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 1024, 'actionHiddenSize': 128})
        with torch.no_grad():
            pol.dist.linear.weight.mul_(100.0)                   # (gain 0.01 leaves the 8 actions all but uniform)
        space = Discrete()
    return enc.to("cuda").eval(), pol.to("cuda"), space, cfg


@functools.lru_cache(maxsize=None)
def env_inputs(which, steps=N_OBSERVE):
    """Step 0 is envs.reset(); steps 1..steps what the simulator returns.  One step carries a new goal, one has every env done."""
    rng = np.random.default_rng(7 if which == "arm" else 8)
    frames = 100 if which == "arm" else 600
    out = []
    for t in range(steps + 1):
        d = dict(image=rng.integers(0, 256, size=(N_ENVS, 3, 96, 96), dtype=np.uint8),
                 env_reward=rng.normal(0, 1.5, size=N_ENVS) * (rng.random(N_ENVS) < 0.6), done=rng.random(N_ENVS) < 0.2,
                 bad=rng.random(N_ENVS) < 0.15, goal=None)
        d["extras"] = ({'robot_pose': rng.normal(size=(N_ENVS, 2)).astype(np.float32)} if which == "arm" else
                       {'occupancy': ((rng.random((N_ENVS, 1, 9, 9)) < 0.3) * 255).astype(np.uint8)})
        if t in (0, GOAL_STEP):
            d["goal"] = rng.normal(size=(N_ENVS, 1, frames, 40)).astype(np.float32)
        if t == ALL_DONE:
            d["done"][:] = True
        out.append(d)
    return out


def storage(var_amd, which, act):
    enc, pol, space, cfg = models(which)
    shapes = {k: tuple(v.shape[1:]) for k, v in act.obs.items()}
    return var_amd.RolloutStorage(T_STEPS, N_ENVS, shapes, space, pol.recurrent_hidden_state_size, cfg, image_dtype=torch.uint8)


def stores_of(ro):
    d = {"obs." + k: v for k, v in ro.obs.items()}
    d.update(hxs=ro.recurrent_hidden_states, rewards=ro.rewards, value_preds=ro.value_preds, logp=ro.action_log_probs, actions=ro.actions,
             masks=ro.masks, bad_masks=ro.bad_masks)
    return d


def snapshot(ro):
    return {k: v.clone() for k, v in stores_of(ro).items()}


def leg_existing_parts(var_amd, which, seed=5):
    """What the library offered before: IntrinsicReward.step, a host read, ReturnNormalizer, tensors back up, insert."""
    enc, pol, space, cfg = models(which)
    ins = env_inputs(which)
    ir = var_amd.IntrinsicReward(enc).capture(N_ENVS)
    act = pol.capture(N_ENVS, seed=seed)
    ro = storage(var_amd, which, act)
    norm = var_amd.ReturnNormalizer(N_ENVS)
    extra = next(iter(ins[0]["extras"]))

    def obs_of(d):
        f, g, dot = ir.step(dev(d["image"]), None if d["goal"] is None else dev(d["goal"]))
        return {'image': dev(d["image"]), extra: dev(d["extras"][extra]), 'image_feat': f, 'goal_sound_feat': g}, dot

    obs, _ = obs_of(ins[0])
    for k in ro.obs:
        ro.obs[k][0].copy_(obs[k])
    masks = torch.ones(N_ENVS, 1, device="cuda")
    snaps, actions = [], []
    for t in range(1, N_OBSERVE + 1):
        value, action, logp, hxs = act(obs, masks)
        actions.append(action.clone())
        d = ins[t]
        obs, dot = obs_of(d)
        rews = dot.cpu().numpy().astype(np.float64) + d["env_reward"]          # the host round trip
        out = norm(rews, d["done"])
        reward = dev(out.astype(np.float32).reshape(-1, 1))
        masks = dev((1.0 - d["done"]).astype(np.float32).reshape(-1, 1))
        bad_masks = dev((1.0 - d["bad"]).astype(np.float32).reshape(-1, 1))
        ro.insert(obs, hxs, action, logp, value, reward, masks, bad_masks)
        if t % T_STEPS == 0 or t == N_OBSERVE:
            snaps.append(snapshot(ro))
            ro.after_update()
    torch.cuda.synchronize()
    return dict(snaps=snaps, actions=torch.stack(actions), state=(float(norm.ret_rms.mean), float(norm.ret_rms.var),
                                                                  float(norm.ret_rms.count), norm.ret.copy()), step=ro.step)


def leg_collect_step(var_amd, which, seed=5, inputs="host inputs"):
    """inputs: "host inputs" (numpy arrays through the pinned block), "device inputs" (CUDA tensors, copied) or "mixed inputs"
    (image and goal on the device, env_reward written in place into the step's own buffer, the rest from the host)."""
    enc, pol, space, cfg = models(which)
    ins = env_inputs(which)
    act = pol.capture(N_ENVS, seed=seed)
    ro = storage(var_amd, which, act)
    cs = var_amd.CollectStep(var_amd.IntrinsicReward(enc), act, ro)
    assert len(cs._segs) == len(act.obs) + 7 <= 16
    to_dev = lambda a: None if a is None else (dev(a.astype(np.uint8)) if a.dtype == np.bool_ else dev(a))   # noqa: E731
    big = to_dev if inputs != "host inputs" else (lambda a: a)
    up = to_dev if inputs == "device inputs" else (lambda a: a)
    upd = lambda e: {k: up(v) for k, v in e.items()}             # noqa: E731

    def env_reward_of(d):
        if inputs != "mixed inputs":
            return up(d["env_reward"])
        cs.env_reward.copy_(dev(d["env_reward"]))
        return cs.env_reward

    cs.reset(big(ins[0]["image"]), upd(ins[0]["extras"]), big(ins[0]["goal"]))
    snaps, actions = [], []
    for t in range(1, N_OBSERVE + 1):
        value, action, logp, hxs = act(act.obs, act.masks)
        actions.append(action.clone())
        d = ins[t]
        done = d["done"].tolist() if inputs == "mixed inputs" else up(d["done"])
        r = cs.observe(big(d["image"]), upd(d["extras"]), env_reward_of(d), done, up(d["bad"]), big(d["goal"]))
        assert r is cs.norm.reward and ro.step == t % T_STEPS
        if t % T_STEPS == 0 or t == N_OBSERVE:
            snaps.append(snapshot(ro))
            ro.after_update()
    torch.cuda.synchronize()
    return dict(snaps=snaps, actions=torch.stack(actions), state=cs.norm.state(), step=ro.step, stats=cs.episode_stats(), cs=cs)


@functools.lru_cache(maxsize=None)
def collect_run(which, run):
    import var_amd
    return leg_collect_step(var_amd, which, inputs=run)


def assert_same_run(a, b):
    assert len(a["snaps"]) == len(b["snaps"]) == 3 and a["step"] == b["step"]
    for sa, sb in zip(a["snaps"], b["snaps"]):
        for k in sa:
            assert sa[k].dtype == sb[k].dtype and np.array_equal(raw(sa[k]), raw(sb[k])), k
    assert np.array_equal(raw(a["actions"]), raw(b["actions"]))
    assert a["state"][:3] == b["state"][:3] and np.array_equal(bits64(a["state"][3]), bits64(b["state"][3]))


@pytest.mark.parametrize("which", ["arm", "ithor"])
def test_collect_step_fills_the_storage_as_the_existing_parts_do(var_amd, which):
    """8 env steps at T = 3: two wraps with after_update in between, a new goal sound at one step, every env done at another."""
    want = leg_existing_parts(var_amd, which)
    got = collect_run(which, "host inputs")
    assert_same_run(got, want)
    assert all(s["rewards"].abs().max() > 0 for s in want["snaps"])
    assert (want["snaps"][1]["masks"][T_STEPS] == 0).all() and any((s["bad_masks"] == 0).any() for s in want["snaps"])
    assert not torch.equal(want["actions"][0], want["actions"][1])
    ins = env_inputs(which)
    finished = sum(d["done"].astype(np.float64) for d in ins[1:])
    assert np.array_equal(got["stats"]["finished"], finished) and finished.min() >= 1


@pytest.mark.parametrize("which", ["arm", "ithor"])
def test_collect_step_built_twice_gives_the_same_bits(var_amd, which):
    """A second and a third CollectStep (fresh ActStep, storage and graphs), fed device tensors instead of host arrays, and a
    mixture with env_reward written in place into the step's own buffer."""
    assert_same_run(collect_run(which, "device inputs"), collect_run(which, "host inputs"))
    assert_same_run(collect_run(which, "mixed inputs"), collect_run(which, "host inputs"))


@pytest.mark.parametrize("which", ["arm", "ithor"])
def test_twenty_replays_of_a_repeated_sequence_are_bit_for_bit(var_amd, which):
    cs = collect_run(which, "host inputs")["cs"]
    ins = env_inputs(which)
    runs = []
    for _ in range(2):
        cs.norm.load(var_amd.ReturnNormalizer(N_ENVS))           # a fresh running variance
        cs.rollouts.step = 0                                     # both runs fill the same slots (reset takes the step over)
        cs.reset(ins[0]["image"], ins[0]["extras"], ins[0]["goal"])
        rewards = []
        for i in range(20):
            d = ins[1 + i % 5]
            rewards.append(cs.observe(d["image"], d["extras"], d["env_reward"], d["done"], d["bad"], d["goal"]).clone())
        runs.append((raw(torch.stack(rewards)), {k: raw(v) for k, v in stores_of(cs.rollouts).items()}, cs.norm.state()))
    (ra, sa, na), (rb, sb, nb) = runs
    assert np.array_equal(ra, rb) and all(np.array_equal(sa[k], sb[k]) for k in sa)
    assert na[:3] == nb[:3] and np.array_equal(bits64(na[3]), bits64(nb[3])) and na[2] > 20 * N_ENVS


def test_refusals_leave_storage_and_state_unchanged(var_amd):
    from var_amd import VarHipError
    enc, pol, space, cfg = models("arm")
    ins = env_inputs("arm")
    cs = collect_run("arm", "host inputs")["cs"]
    ro, d = cs.rollouts, ins[1]

    def everything():
        s = {k: raw(v) for k, v in stores_of(ro).items()}
        s.update(f64=raw(cs.norm._f64), slot=raw(cs.norm.slot), masks_buf=raw(cs.act_step.masks), image_buf=raw(cs.act_step.obs['image']))
        return s

    before, step = everything(), ro.step
    with pytest.raises(VarHipError):                             # a wrong image size
        cs.observe(d["image"][:, :, :84, :84], d["extras"], d["env_reward"], d["done"])
    with pytest.raises(VarHipError):
        cs.observe(dev(d["image"])[:, :, :84, :84].contiguous(), d["extras"], d["env_reward"], d["done"])
    with pytest.raises(VarHipError):                             # float images into a uint8 step
        cs.observe(d["image"].astype(np.float32), d["extras"], d["env_reward"], d["done"])
    with pytest.raises(VarHipError):
        cs.observe(d["image"], {}, d["env_reward"], d["done"])
    with pytest.raises(VarHipError):                             # a CPU tensor where the normaliser takes device tensors
        cs.norm(torch.zeros(N_ENVS), torch.zeros(N_ENVS, dtype=torch.float64), torch.zeros(N_ENVS, dtype=torch.uint8))
    with pytest.raises(VarHipError):
        cs.norm(torch.zeros(N_ENVS, device="cuda"), torch.zeros(N_ENVS, dtype=torch.float64, device="cuda"), torch.zeros(N_ENVS, dtype=torch.uint8))
    after = everything()
    assert ro.step == step and all(np.array_equal(before[k], after[k]) for k in before)
    # an insert slipped in between: the device slot no longer is the storage's step
    act = cs.act_step
    ro.insert(act.obs, act._hout, act.action, act.action_log_probs, act.value, cs.norm.reward, act.masks, cs.norm.bad_masks)
    before, step = everything(), ro.step
    with pytest.raises(VarHipError, match="insert"):
        cs.observe(d["image"], d["extras"], d["env_reward"], d["done"])
    after = everything()
    assert ro.step == step and all(np.array_equal(before[k], after[k]) for k in before)
    cs.reset(ins[0]["image"], ins[0]["extras"], ins[0]["goal"])  # reset takes the storage's step over
    cs.observe(d["image"], d["extras"], d["env_reward"], d["done"])
    assert ro.step == (step + 1) % T_STEPS
    # what the constructor refuses
    enc84 = var_amd.VARPretextNet(types.SimpleNamespace(img_dim=(3, 84, 84), sound_dim=(1, 100, 40), representationDim=3)).to("cuda")
    with pytest.raises(VarHipError, match="images"):
        var_amd.CollectStep(var_amd.IntrinsicReward(enc84), act, ro)
    f32_store = var_amd.RolloutStorage(T_STEPS, N_ENVS, {k: tuple(v.shape[1:]) for k, v in act.obs.items()}, space, 512, cfg)
    with pytest.raises(VarHipError, match="image dtype"):
        var_amd.CollectStep(var_amd.IntrinsicReward(enc), act, f32_store)
    cpu_enc = var_amd.VARPretextNet(types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 100, 40), representationDim=3))
    with pytest.raises(VarHipError):
        var_amd.CollectStep(var_amd.IntrinsicReward(cpu_enc), act, ro)
    with pytest.raises(VarHipError):
        var_amd.CollectStep(var_amd.IntrinsicReward(enc), types.SimpleNamespace(), ro)
    with pytest.raises(VarHipError):
        var_amd.DeviceReturnNormalizer(129)

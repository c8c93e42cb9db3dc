"""GPU checks of the sound-sound reward term (config.RLRewardSoundSound; Envs/vec_env/vec_pretext_normalize.py:82-101):
var_reward_dots, var_ithor_reward_plan_ex / var_ithor_reward_step_ex, IntrinsicReward(model, sound_sound=True).capture and
CollectStep on such a reward.

Bounds.  One: the current clips' embedding against the CPU checker at ATOL_CHECKER = 1e-4, the bound
tests/test_gpu_ithor_reward.py holds goal_feat to on the same kernels.  Everything else is bit for bit: the dots against the
numpy restatement of tests/sound_sound_cpu.py (pinned to IntrinsicReward.reward by tests/test_sound_sound_host.py; products and
adds are IEEE float32 operations, the library is built without contraction); a current clip's embedding against the goal_feat
the existing entry writes for the same clip at the same B (same kernels, a clip never mixes with another); replays against
eager calls; CollectStep against the same parts wired by hand (same kernels on the same bits, then host float64 in the
reference's grouping)."""
import functools
import types

import numpy as np
import pytest
import torch

from tests import _ithor_reward_inputs as rin
from tests import sound_sound_cpu as ss

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_PLAN = -1, -3
ATOL_CHECKER = 1e-4
NAN = float("nan")
IMG_FLOATS = 3 * 96 * 96
SOUND_SOUND = 1                                                  # VAR_IREW_SOUND_SOUND


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.set_num_threads(8)
    return m


@pytest.fixture(scope="module")
def ctx(var_amd):
    from var_amd._lib import Context
    return Context.get(0)


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def p(t):
    return None if t is None else t.data_ptr()


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def raw(t):
    return host(t.contiguous().view(-1).view(torch.uint8))


def nans(*shape):
    return torch.full(shape, NAN, device="cuda")


def all_nan(*ts):
    torch.cuda.synchronize()
    return all(bool(torch.isnan(t).all()) for t in ts)


def stream():
    from var_amd._lib import current_stream_handle
    return current_stream_handle()


# ---- var_reward_dots --------------------------------------------------------------------------------------------------------
def dots(c, img, goal, cur, rows, dim, out, out_img, out_snd):
    return c.lib.var_reward_dots(c.handle, stream(), p(img), p(goal), p(cur), rows, dim, p(out), p(out_img), p(out_snd))


@pytest.mark.parametrize("dim", [3, 64])
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_reward_dots_equal_the_restatement_bit_for_bit(ctx, rows, dim):
    """rows around the 256-thread block edge; dim 3 (the embeddings) and 64 (the entry's limit)."""
    img, goal, cur = ss.unit_rows(rows, dim, seed=100 * dim + rows)
    d_img, d_goal, d_cur = cuda(img), cuda(goal), cuda(cur)
    out, a, b = nans(rows), nans(rows), nans(rows)
    assert dots(ctx, d_img, d_goal, d_cur, rows, dim, out, a, b) == 0, ctx.lib.var_last_error(ctx.handle)
    w_out, w_a, w_b = ss.reward_dots(img, goal, cur)
    assert np.array_equal(bits32(host(out)), bits32(w_out))
    assert np.array_equal(bits32(host(a)), bits32(w_a)) and np.array_equal(bits32(host(b)), bits32(w_b))
    only = nans(rows)                                            # the two optional outputs left out
    assert dots(ctx, d_img, d_goal, d_cur, rows, dim, only, None, None) == 0
    assert np.array_equal(bits32(host(only)), bits32(w_out))
    # no second term: var_row_dot's bits
    out0, a0, b0, rd = nans(rows), nans(rows), nans(rows), nans(rows)
    assert dots(ctx, d_img, d_goal, None, rows, dim, out0, a0, b0) == 0
    assert ctx.lib.var_row_dot(ctx.handle, stream(), p(d_img), p(d_goal), rows, dim, p(rd)) == 0
    assert np.array_equal(bits32(host(out0)), bits32(host(rd))) and np.array_equal(bits32(host(a0)), bits32(host(rd)))
    assert np.array_equal(bits32(host(rd)), bits32(ss.row_dot(img, goal))) and not host(b0).any()


def test_reward_dots_refuses_bad_arguments_and_writes_nothing(ctx):
    rows, dim = 5, 3
    img, goal, cur = (cuda(a) for a in ss.unit_rows(rows, 65, seed=1))
    out, a, b = nans(rows), nans(rows), nans(rows)
    assert dots(ctx, img, goal, cur, 0, dim, out, a, b) == ERR_ARG
    assert b"var_reward_dots" in ctx.lib.var_last_error(ctx.handle)
    assert dots(ctx, img, goal, cur, rows, 65, out, a, b) == ERR_ARG
    assert dots(ctx, img, goal, cur, rows, 0, out, a, b) == ERR_ARG
    assert dots(ctx, None, goal, cur, rows, dim, out, a, b) == ERR_ARG
    assert dots(ctx, img, None, cur, rows, dim, out, a, b) == ERR_ARG
    assert dots(ctx, img, goal, cur, rows, dim, None, a, b) == ERR_ARG
    assert all_nan(out, a, b)
    assert dots(ctx, img, goal, cur, rows, dim, out, a, b) == 0 and not all_nan(out)


# ---- the iTHOR reward step --------------------------------------------------------------------------------------------------
def cfg96():
    return types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 600, 40), representationDim=3)


@functools.lru_cache(maxsize=None)
def ithor_encoder():
    """(checker, HIP model) with the spread heads of tests/_ithor_reward_inputs.py."""
    import var_amd
    ref = rin.spread_checker()
    m = var_amd.IthorVARPretextNet(cfg96())
    m.load_state_dict(ref.state_dict())
    return ref, m.to("cuda").eval()


class OwnContext:
    """A context of its own, planned with var_ithor_reward_plan_ex(batch, 96, flags) and packed: the plan is exactly what the
    test asked for, whatever the process-wide context has grown to."""

    def __init__(self, flat, batch, flags):
        from var_amd._lib import Context
        self.flat, self.batch, self.flags = flat, batch, flags
        self.c = Context(0)

    def __enter__(self):
        c = self.c
        assert c.lib.var_ithor_reward_plan_ex(c.handle, self.batch, 96, self.flags) == 0, c.lib.var_last_error(c.handle)
        assert c.lib.var_ithor_reward_pack(c.handle, stream(), p(self.flat)) == 0, c.lib.var_last_error(c.handle)
        return c

    def __exit__(self, *exc):
        torch.cuda.synchronize()
        self.c.lib.var_destroy(self.c.handle)
        self.c.handle = None


def step(c, flat, image, goal, B, image_feat, goal_feat, reward):
    return c.lib.var_ithor_reward_step(c.handle, stream(), p(flat), p(image), 1, image.stride(0), p(goal), B, p(image_feat),
                                       p(goal_feat), p(reward))


def step_ex(c, flat, image, goal, cur, B, image_feat, goal_feat, cur_feat, reward, reward_img, reward_snd):
    return c.lib.var_ithor_reward_step_ex(c.handle, stream(), p(flat), p(image), 1, image.stride(0), p(goal), p(cur), B,
                                          p(image_feat), p(goal_feat), p(cur_feat), p(reward), p(reward_img), p(reward_snd))


def ex_outs(B):
    return dict(image_feat=nans(B, 3), goal_feat=nans(B, 3), cur_feat=nans(B, 3), reward=nans(B), reward_img=nans(B), reward_snd=nans(B))


def current_clips(B, seed, zero_clip):
    cur = rin.spread_sounds(B, seed)
    if zero_clip is not None:
        cur[zero_clip] = 0.0
    return cur


def test_step_ex_without_current_clips_is_the_existing_step(var_amd):
    """cur_mfcc = NULL, on a goal step and on an image-only step at B = 8: var_ithor_reward_step's bits; cur_feat and the two
    optional outputs stay as they were."""
    _, m = ithor_encoder()
    flat, B = m.flat_parameters(), 8
    img, snd = (cuda(a) for a in rin.spread_inputs(B))
    img2 = cuda(rin.spread_images(B, 31))
    with OwnContext(flat, B, SOUND_SOUND) as c:
        want = [nans(B, 3), nans(B, 3), nans(B)]
        o = ex_outs(B)
        for image, goal in ((img, snd), (img2, None)):
            assert step(c, flat, image, goal, B, *want) == 0, c.lib.var_last_error(c.handle)
            assert step_ex(c, flat, image, goal, None, B, **o) == 0, c.lib.var_last_error(c.handle)
            torch.cuda.synchronize()
            assert torch.equal(o["image_feat"], want[0]) and torch.equal(o["goal_feat"], want[1]) and torch.equal(o["reward"], want[2])
            assert bool(torch.isfinite(want[2]).all()) and all_nan(o["cur_feat"], o["reward_img"], o["reward_snd"])


@pytest.mark.parametrize("B,plan", [(1, 1), (8, 8), (9, 9), (16, 16), (17, 64)])
def test_step_ex_with_current_clips(var_amd, B, plan):
    """B = 8: the merge limit 2B = 16 (goal and current clips in one pass, 16 columns of the fused GRU step); 9: one above it
    (two passes); 16: the fused kernel's limit; 17 under a 64-env plan: the two-launch GRU route; 1: the smallest plan (two
    rows).  A goal step and a current-only step, one current clip all zero, every output NaN before."""
    _, m = ithor_encoder()
    flat = m.flat_parameters()
    img, snd = (cuda(a) for a in rin.spread_inputs(B))
    img2 = cuda(rin.spread_images(B, 31))
    cur = cuda(current_clips(B, 22, min(3, B - 1)))
    cur2 = cuda(current_clips(B, 23, 0 if B > 1 else None))
    with OwnContext(flat, plan, SOUND_SOUND) as c:
        # what the existing entry gives: the clips as goal clips at the same B, and the two steps without a current sound
        as_goal, as_goal2, g_ref, g_ref2 = nans(B, 3), nans(B, 3), nans(B, 3), nans(B, 3)
        i_ref, i_ref2, w_ref, w_ref2, scratch_i, scratch_w = nans(B, 3), nans(B, 3), nans(B), nans(B), nans(B, 3), nans(B)
        assert step(c, flat, img, cur, B, scratch_i, as_goal, scratch_w) == 0, c.lib.var_last_error(c.handle)
        assert step(c, flat, img, cur2, B, scratch_i, as_goal2, scratch_w) == 0
        assert step(c, flat, img, snd, B, i_ref, g_ref, w_ref) == 0
        g_ref2.copy_(g_ref)
        assert step(c, flat, img2, None, B, i_ref2, g_ref2, w_ref2) == 0
        o = ex_outs(B)
        for image, goal, clips, want_i, want_g, want_c, want_w in ((img, snd, cur, i_ref, g_ref, as_goal, w_ref),
                                                                   (img2, None, cur2, i_ref2, g_ref2, as_goal2, w_ref2)):
            if goal is None:
                for k in ("image_feat", "cur_feat", "reward", "reward_img", "reward_snd"):
                    o[k].fill_(NAN)                              # (goal_feat carries the cached embedding)
            assert step_ex(c, flat, image, goal, clips, B, **o) == 0, c.lib.var_last_error(c.handle)
            torch.cuda.synchronize()
            what = "goal step" if goal is not None else "current-only step"
            assert torch.equal(o["cur_feat"], want_c), f"{what}: cur_feat is not the clips' goal_feat at B = {B}"
            assert torch.equal(o["image_feat"], want_i) and torch.equal(o["goal_feat"], want_g), what
            assert torch.equal(o["reward_img"], want_w), what
            r, ri, rs = host(o["reward"]), host(o["reward_img"]), host(o["reward_snd"])
            assert np.isfinite(r).all() and np.array_equal(bits32(r), bits32((ri + rs).astype(np.float32))), what
            w_out, w_a, w_b = ss.reward_dots(host(o["image_feat"]), host(o["goal_feat"]), host(o["cur_feat"]))
            assert np.array_equal(bits32(r), bits32(w_out)) and np.array_equal(bits32(rs), bits32(w_b)), what
            assert np.abs(rs).max() > 0
            only = nans(B)                                       # the two optional outputs left out
            assert step_ex(c, flat, image, goal, clips, B, o["image_feat"], o["goal_feat"], o["cur_feat"], only, None, None) == 0
            assert np.array_equal(bits32(host(only)), bits32(r)), what
        assert not torch.equal(as_goal, as_goal2)


def test_current_clips_against_the_cpu_checker(var_amd):
    ref, m = ithor_encoder()
    flat, B = m.flat_parameters(), 8
    img = cuda(rin.spread_images(B))
    clips = rin.spread_sounds(B)
    want = rin.checker_goal_feat(ref, clips)
    assert rin.min_row_distance(want) >= rin.MIN_ROW_DISTANCE
    goal = cuda(current_clips(B, 22, None))
    with OwnContext(flat, B, SOUND_SOUND) as c:
        o = ex_outs(B)
        assert step_ex(c, flat, img, goal, cuda(clips), B, **o) == 0, c.lib.var_last_error(c.handle)
        merged = host(o["cur_feat"])
        o["cur_feat"].fill_(NAN)
        assert step_ex(c, flat, img, None, cuda(clips), B, **o) == 0
        alone = host(o["cur_feat"])
    print(f"cur_feat vs checker: merged pass {np.abs(merged - want).max():.2e}, a pass of its own {np.abs(alone - want).max():.2e}")
    np.testing.assert_allclose(merged, want, atol=ATOL_CHECKER, rtol=0)
    assert np.array_equal(bits32(merged), bits32(alone))


def test_current_clips_need_the_plans_bit_and_a_cur_feat(var_amd):
    _, m = ithor_encoder()
    flat, B = m.flat_parameters(), 8
    img, snd = (cuda(a) for a in rin.spread_inputs(B))
    with OwnContext(flat, B, 0) as c:                            # var_ithor_reward_plan_ex without bit 0
        o = ex_outs(B)
        assert step_ex(c, flat, img, snd, snd, B, **o) == ERR_PLAN
        assert b"VAR_IREW_SOUND_SOUND" in c.lib.var_last_error(c.handle)
        assert step_ex(c, flat, img, None, snd, B, **o) == ERR_PLAN and all_nan(*o.values())
        assert c.lib.var_ithor_reward_plan_ex(c.handle, B, 96, 2) == ERR_ARG
        assert step_ex(c, flat, img, snd, None, B, **o) == 0 and not all_nan(o["reward"])      # (the plan serves the off mode)
        # asking for the bit replaces the plan: pack again, then the step runs
        assert c.lib.var_ithor_reward_plan_ex(c.handle, B, 96, SOUND_SOUND) == 0
        assert c.lib.var_ithor_reward_pack(c.handle, stream(), p(flat)) == 0
        o = ex_outs(B)
        assert step_ex(c, flat, img, snd, snd, B, o["image_feat"], o["goal_feat"], None, o["reward"], None, None) == ERR_ARG
        assert all_nan(*o.values())
        assert step_ex(c, flat, img, snd, snd, B, **o) == 0
        torch.cuda.synchronize()
        assert torch.equal(o["cur_feat"], o["goal_feat"])        # the same clips on both sides of one merged pass


def test_twenty_replays_equal_eager_calls_bit_for_bit(var_amd, ctx):
    """capture(8) with sound_sound: a goal step (the merged 16-clip pass) every fourth step, current-only steps between."""
    _, m = ithor_encoder()
    B = 8
    r = var_amd.IntrinsicReward(m, sound_sound=True).capture(B)
    flat = m.flat_parameters()
    gen = torch.Generator(device="cuda").manual_seed(78)
    e = ex_outs(B)
    for k in range(20):
        img = torch.randint(0, 256, (B, 3, 96, 96), dtype=torch.uint8, device="cuda", generator=gen)
        sounds = torch.randn((2, B, 1, 600, 40), device="cuda", generator=gen) * 6.0
        sounds[:, :, :, :, 0] += 18.0
        sounds[1, k % B, :, 100 + k:] = 0.0
        goal = sounds[0] if k % 4 == 0 else None
        if goal is None:
            e["goal_feat"].copy_(r._goal_feat)
        i, g, w = r.step(img, goal, sounds[1])
        assert step_ex(ctx, flat, img, goal, sounds[1], B, **e) == 0, ctx.lib.var_last_error(ctx.handle)
        torch.cuda.synchronize()
        same = (torch.equal(i, e["image_feat"]) and torch.equal(g, e["goal_feat"]) and torch.equal(w, e["reward"]) and
                torch.equal(r.cur_feat, e["cur_feat"]) and torch.equal(r.img_sound_dot, e["reward_img"]) and
                torch.equal(r.sound_sound_dot, e["reward_snd"]))
        assert same, f"replay {k} differs from the eager call"
        assert bool(torch.isfinite(w).all())
    with pytest.raises(var_amd.VarHipError, match="current_sound"):
        r.step(img, None, None)
    with pytest.raises(var_amd.VarHipError):
        r.step(img, None, sounds[1].cpu())
    torch.cuda.synchronize()
    assert torch.equal(w, e["reward"])                           # (the refused steps replayed nothing)


# ---- the Kuka encoder -------------------------------------------------------------------------------------------------------
def kuka_model(golden_dir, hw):
    import os
    import var_amd
    sd = dict(np.load(os.path.join(golden_dir, "kuka_weights.npz")))
    m = var_amd.VARPretextNet(types.SimpleNamespace(img_dim=(3, hw, hw), sound_dim=(1, 100, 40), representationDim=3))
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to("cuda")


@pytest.mark.parametrize("hw", [96, 84])
def test_kuka_capture_with_sound_sound(var_amd, ctx, golden_dir, hw):
    """96: the RL stage's size; 84: where the off mode's image-only graph lets the image head take the dot itself -- with the
    second term on no dot is armed, the reward is var_reward_dots' sum of both."""
    B = 8
    m = kuka_model(golden_dir, hw)
    r = var_amd.IntrinsicReward(m, sound_sound=True).capture(B)
    rng = np.random.default_rng(hw)
    img1, img2 = (cuda(rng.integers(0, 256, size=(B, 3, hw, hw), dtype=np.uint8)) for _ in range(2))
    goal, cur1, cur2 = (cuda(rng.standard_normal((B, 1, 100, 40)).astype(np.float32)) for _ in range(3))
    flat = m.flat_parameters()
    g_first = None
    for image, g_in, cur in ((img1, goal, cur1), (img2, None, cur2)):
        f, g, w = r.step(image, g_in, cur)
        f, g, w, cf = host(f), host(g), host(w), host(r.cur_feat)
        feat, neg = nans(B, 3), nans(B, 3)
        ctx.ensure_plan(B, hw)
        m.hip_weights(ctx).bind()
        ctx.check(ctx.lib.var_arm_encoder_fwd(ctx.handle, stream(), p(flat), p(image), 1, image.stride(0), None, p(cur), B, hw, p(feat), None,
                                              p(neg), None, None, 2), "var_arm_encoder_fwd")
        assert np.array_equal(bits32(cf), bits32(host(neg))) and np.array_equal(bits32(f), bits32(host(feat)))
        w_out, w_a, w_b = ss.reward_dots(f, g, cf)
        assert np.array_equal(bits32(w), bits32(w_out)), "reward is not the restatement on the downloaded embeddings"
        assert np.array_equal(bits32(host(r.img_sound_dot)), bits32(w_a)) and np.array_equal(bits32(host(r.sound_sound_dot)), bits32(w_b))
        assert np.abs(w_b).max() > 0 and not np.array_equal(bits32(w), bits32(w_a))          # (not the off mode's dot alone)
        if g_first is None:
            g_first = g
        assert np.array_equal(g, g_first), "the cached goal embedding changed in a current-only step"
    before = raw(r._img), raw(r.current_sound), raw(r._reward)
    with pytest.raises(var_amd.VarHipError, match="current_sound"):
        r.step(img1, goal)                                       # refused before anything is copied or replayed
    assert all(np.array_equal(a, b) for a, b in zip(before, (raw(r._img), raw(r.current_sound), raw(r._reward))))
    # off: current_sound is ignored, every existing call gives the bits it gives today
    off = var_amd.IntrinsicReward(m).capture(B)
    a = [host(t) for t in off.step(img1, goal, cur1)]
    b = [host(t) for t in off.step(img1, goal)]
    assert all(np.array_equal(bits32(x), bits32(y)) for x, y in zip(a, b)) and off.current_sound is None
    assert np.array_equal(bits32(a[2]), bits32(ss.row_dot(a[0], a[1])))


# ---- CollectStep ------------------------------------------------------------------------------------------------------------
N_ENVS, T_STEPS, N_OBSERVE, GOAL_STEP, DONE_STEP = 8, 4, 6, 3, 2


class Discrete:
    def __init__(self, n=8):
        self.n = n


class Box:
    def __init__(self, n=2):
        self.shape = (n,)


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
        enc = var_amd.IthorVARPretextNet(cfg96())
        cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, RLObsIgnore=[])
        pol = var_amd.IthorNetPolicy(None, Discrete(), config=cfg, base='ai2thor_VAR', base_kwargs={
            'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 1024, 'actionHiddenSize': 128})
        with torch.no_grad():
            pol.dist.linear.weight.mul_(100.0)                   # (gain 0.01 leaves the 8 actions all but uniform)
        space = Discrete()
    return enc.to("cuda").eval(), pol.to("cuda"), space, cfg


@functools.lru_cache(maxsize=None)
def env_inputs(which):
    """Step 0 is envs.reset(); steps 1..N_OBSERVE what the simulator returns, each with its current sound.  One step carries a
    new goal, one has an env done."""
    rng = np.random.default_rng(17 if which == "arm" else 18)
    frames = 100 if which == "arm" else 600
    out = []
    for t in range(N_OBSERVE + 1):
        d = dict(image=rng.integers(0, 256, size=(N_ENVS, 3, 96, 96), dtype=np.uint8),
                 env_reward=rng.normal(0, 1.5, size=N_ENVS) * (rng.random(N_ENVS) < 0.6), done=np.zeros(N_ENVS, bool),
                 bad=rng.random(N_ENVS) < 0.15, goal=None, current=rng.normal(size=(N_ENVS, 1, frames, 40)).astype(np.float32))
        d["extras"] = ({'robot_pose': rng.normal(size=(N_ENVS, 2)).astype(np.float32)} if which == "arm" else
                       {'occupancy': ((rng.random((N_ENVS, 1, 9, 9)) < 0.3) * 255).astype(np.uint8)})
        if t in (0, GOAL_STEP):
            d["goal"] = rng.normal(size=(N_ENVS, 1, frames, 40)).astype(np.float32)
        if t == DONE_STEP:
            d["done"][5] = True
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
    return {k: raw(v) for k, v in stores_of(ro).items()}


def leg_by_hand(var_amd, which, seed=5):
    """The captured IntrinsicReward.step, the embeddings read back, host IntrinsicReward.reward + ReturnNormalizer, then
    RolloutStorage.insert; the episode block as RL.py:171-176 keeps it."""
    enc, pol, space, cfg = models(which)
    ins = env_inputs(which)
    ir = var_amd.IntrinsicReward(enc, sound_sound=True).capture(N_ENVS)
    act = pol.capture(N_ENVS, seed=seed)
    ro = storage(var_amd, which, act)
    norm = var_amd.ReturnNormalizer(N_ENVS)
    extra = next(iter(ins[0]["extras"]))
    episode = np.zeros((3, N_ENVS))

    def obs_of(d):
        f, g, _ = ir.step(cuda(d["image"]), None if d["goal"] is None else cuda(d["goal"]), cuda(d["current"]))
        obs = {'image': cuda(d["image"]), extra: cuda(d["extras"][extra]), 'image_feat': f, 'goal_sound_feat': g}
        return obs, (host(f), host(g), host(ir.cur_feat))

    obs, _ = obs_of(ins[0])                                      # (the reset's reward is discarded)
    for k in ro.obs:
        ro.obs[k][0].copy_(obs[k])
    masks = torch.ones(N_ENVS, 1, device="cuda")
    snaps, dots = [], []
    for t in range(1, N_OBSERVE + 1):
        value, action, logp, hxs = act(obs, masks)
        d = ins[t]
        obs, (f, g, cf) = obs_of(d)
        rews, img_dot, snd_dot = ir.reward(d["env_reward"], f, g, cf)                # the host round trip
        assert rews.dtype == np.float64 and np.abs(snd_dot).max() > 0
        dots.append((img_dot, snd_dot))
        out = norm(rews, d["done"])
        run = episode[0] + rews
        episode[1][d["done"]] = run[d["done"]]
        episode[2] += d["done"]
        run[d["done"]] = 0.0
        episode[0] = run
        reward = cuda(out.astype(np.float32).reshape(-1, 1))
        masks = cuda((1.0 - d["done"]).astype(np.float32).reshape(-1, 1))
        bad_masks = cuda((1.0 - d["bad"]).astype(np.float32).reshape(-1, 1))
        ro.insert(obs, hxs, action, logp, value, reward, masks, bad_masks)
        if t % T_STEPS == 0 or t == N_OBSERVE:
            snaps.append(snapshot(ro))
            ro.after_update()
    torch.cuda.synchronize()
    return dict(snaps=snaps, state=(float(norm.ret_rms.mean), float(norm.ret_rms.var), float(norm.ret_rms.count), norm.ret.copy()),
                step=ro.step, episode=episode, dots=dots)


def leg_collect_step(var_amd, which, seed=5):
    enc, pol, space, cfg = models(which)
    ins = env_inputs(which)
    act = pol.capture(N_ENVS, seed=seed)
    ro = storage(var_amd, which, act)
    cs = var_amd.CollectStep(var_amd.IntrinsicReward(enc, sound_sound=True), act, ro)
    assert tuple(cs.current_sound.shape) == tuple(cs.goal_sound.shape) and cs._stage['current_sound'][0] % 16 == 0
    cs.reset(ins[0]["image"], ins[0]["extras"], ins[0]["goal"])
    snaps, dots, refusal = [], [], None
    for t in range(1, N_OBSERVE + 1):
        act(act.obs, act.masks)
        d = ins[t]
        if t == T_STEPS + 1:                                     # behind the slot wrap: a step without its current sound
            def everything():
                s = snapshot(ro)
                s.update(f64=raw(cs.norm._f64), slot=raw(cs.norm.slot), masks_buf=raw(act.masks), image_buf=raw(act.obs['image']),
                         cur_buf=raw(cs.current_sound), dot=raw(cs.dot))
                return s
            before, step_before = everything(), ro.step
            with pytest.raises(var_amd.VarHipError, match="current_sound"):
                cs.observe(d["image"], d["extras"], d["env_reward"], d["done"], d["bad"], d["goal"])
            after = everything()
            refusal = ro.step == step_before and all(np.array_equal(before[k], after[k]) for k in before)
        # host arrays on even steps, device tensors on odd ones, once the step's own buffer in place
        cur = d["current"] if t % 2 == 0 else cuda(d["current"])
        if t == 3:
            cs.current_sound.copy_(cuda(d["current"]))
            cur = cs.current_sound
        r = cs.observe(d["image"], d["extras"], d["env_reward"], d["done"], d["bad"], d["goal"], cur)
        assert r is cs.norm.reward and ro.step == t % T_STEPS
        dots.append((host(cs.dot_img), host(cs.dot_snd), host(cs.dot), host(cs.cur_feat)))
        if t % T_STEPS == 0 or t == N_OBSERVE:
            snaps.append(snapshot(ro))
            ro.after_update()
    torch.cuda.synchronize()
    return dict(snaps=snaps, state=cs.norm.state(), step=ro.step, stats=cs.episode_stats(), dots=dots, refusal=refusal)


@pytest.mark.parametrize("which", ["arm", "ithor"])
def test_collect_step_with_sound_sound_equals_the_parts_wired_by_hand(var_amd, which):
    """N = 8, T = 4, six observes: across the slot wrap, one env done at step 2, a new goal at step 3 (on iTHOR the merged
    16-clip pass)."""
    want = leg_by_hand(var_amd, which)
    got = leg_collect_step(var_amd, which)
    assert len(got["snaps"]) == len(want["snaps"]) == 2 and got["step"] == want["step"] == N_OBSERVE % T_STEPS
    for sa, sb in zip(got["snaps"], want["snaps"]):
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), k
    assert got["state"][:3] == want["state"][:3] and np.array_equal(bits64(got["state"][3]), bits64(want["state"][3]))
    stats = got["stats"]
    for row, key in enumerate(("running", "last", "finished")):
        assert np.array_equal(bits64(stats[key]), bits64(want["episode"][row])), key
    assert stats["finished"].sum() == 1
    for (di, ds, dsum, _), (wi, ws) in zip(got["dots"], want["dots"]):
        assert np.array_equal(bits32(di), bits32(wi)) and np.array_equal(bits32(ds), bits32(ws))
        assert np.array_equal(bits32(dsum), bits32((wi + ws).astype(np.float32)))
    assert got["refusal"] is True, "a step refused for its missing current_sound changed the storage, the normaliser or the slot"

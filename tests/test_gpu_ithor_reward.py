"""GPU tests of the frozen iTHOR encoder's reward step (var_ithor_reward_plan / _pack / _step, IntrinsicReward.capture on an
IthorVARPretextNet), each through ctypes / IntrinsicReward only.

Checker: oracle.torch_oracle.IthorNetCPU (pinned to the reference by tests/golden/ithor_h96.npz through
tests/test_oracle_ithor.py) and that fixture itself at B = 2.  Inputs and head weights are the spread recipe of
tests/_ithor_reward_inputs.py, on which the checker's rows are >= 2e-3 apart (asserted here on the checker's output).
Tolerances, all the project's own: embeddings atol 1e-4 against the checker (tests/test_gpu_ithor.py holds this model to it
against the reference fixture; the checker's float32-vs-float64 distance on these inputs is 1.6e-7); reward atol 1e-6
against the float64 dot of the RETURNED embeddings (three fp32 products of unit vectors); old path vs new path atol 2e-5
(test_large_ragged_batch_is_consistent_with_its_parts uses that between two summation orders of this model)."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import _ithor_reward_inputs as rin  # noqa: E402

ATOL_CHECKER, ATOL_DOT, ATOL_PATHS = 1e-4, 1e-6, 2e-5
IMG_FLOATS = 3 * 96 * 96


def cfg(h=96):
    return types.SimpleNamespace(img_dim=(3, h, h), sound_dim=(1, 600, 40), representationDim=3)


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.set_num_threads(8)
    return m


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ithor_h96.npz")))


@pytest.fixture(scope="module")
def ref():
    return rin.spread_checker()


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def hip_model(var_amd, checker):
    m = var_amd.IthorVARPretextNet(cfg())
    m.load_state_dict(checker.state_dict())
    return m.to("cuda").eval()


def host(*ts):
    torch.cuda.synchronize()
    return [t.cpu().numpy().copy() for t in ts]


def assert_reward_is_the_dot(image_feat, goal_feat, reward):
    want = np.sum(image_feat.astype(np.float64) * goal_feat.astype(np.float64), axis=1)
    np.testing.assert_allclose(reward, want, atol=ATOL_DOT, rtol=0)


def raw_step(c, flat, image, goal, B, image_feat, goal_feat, reward, bstride=None):
    """var_ithor_reward_step through ctypes on the current stream; returns the code."""
    from var_amd._lib import current_stream_handle, ptr
    return c.lib.var_ithor_reward_step(c.handle, current_stream_handle(), ptr(flat), ptr(image),
                                       int(image is not None and image.dtype == torch.uint8),
                                       (image.stride(0) if bstride is None else bstride) if image is not None else IMG_FLOATS,
                                       ptr(goal), B, ptr(image_feat), ptr(goal_feat), ptr(reward))


def outs(B, fill=0.0):
    return (torch.full((B, 3), fill, device="cuda"), torch.full((B, 3), fill, device="cuda"), torch.full((B,), fill, device="cuda"))


# ---- 1 ---------------------------------------------------------------------------------------------------------------
def test_fixture_batch_through_capture(var_amd, fx):
    torch.manual_seed(int(fx["seed"]))
    m = var_amd.IthorVARPretextNet(cfg()).to("cuda").eval()
    r = var_amd.IntrinsicReward(m).capture(2)
    i, g, w = host(*r.step(cuda(fx["image"]), cuda(fx["sound_positive"])))
    print("fixture: max |image_feat - ref|", np.abs(i - fx["image_feat"]).max(), " max |goal_feat - ref|",
          np.abs(g - fx["sound_feat_positive"]).max())
    np.testing.assert_allclose(i, fx["image_feat"], atol=ATOL_CHECKER, rtol=0)
    np.testing.assert_allclose(g, fx["sound_feat_positive"], atol=ATOL_CHECKER, rtol=0)
    assert_reward_is_the_dot(i, g, w)


# ---- 2 ---------------------------------------------------------------------------------------------------------------
def test_goal_step_then_image_only_steps_vs_checker(var_amd, ref):
    m = hip_model(var_amd, ref)
    r = var_amd.IntrinsicReward(m).capture(8)
    img, snd = rin.spread_inputs(8)
    want_i, want_g = rin.checker_image_feat(ref, img), rin.checker_goal_feat(ref, snd)
    assert rin.min_row_distance(want_i) >= rin.MIN_ROW_DISTANCE and rin.min_row_distance(want_g) >= rin.MIN_ROW_DISTANCE
    i, g, w = host(*r.step(cuda(img), cuda(snd)))
    print("goal step: max |image_feat - checker|", np.abs(i - want_i).max(), " max |goal_feat - checker|", np.abs(g - want_g).max())
    np.testing.assert_allclose(i, want_i, atol=ATOL_CHECKER, rtol=0)
    np.testing.assert_allclose(g, want_g, atol=ATOL_CHECKER, rtol=0)
    assert_reward_is_the_dot(i, g, w)
    assert w.max() - w.min() > 0.1                               # (the rewards of this recipe are spread, not one value)
    for seed in (31, 32, 33):
        img2 = rin.spread_images(8, seed)
        want2 = rin.checker_image_feat(ref, img2)
        assert rin.min_row_distance(want2) >= rin.MIN_ROW_DISTANCE
        i2, g2, w2 = host(*r.step(cuda(img2)))
        print(f"image-only step (seed {seed}): max |image_feat - checker|", np.abs(i2 - want2).max())
        np.testing.assert_allclose(i2, want2, atol=ATOL_CHECKER, rtol=0)
        assert np.array_equal(g2, g), "the cached goal embedding changed in an image-only step"
        assert_reward_is_the_dot(i2, g2, w2)


# ---- 3 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3, 8, 16, 64])
def test_new_path_equals_the_training_forward(var_amd, ref, B):
    m = hip_model(var_amd, ref)
    img, snd = rin.spread_inputs(B)
    img2 = rin.spread_images(B, 31)
    with torch.no_grad():
        d = m(cuda(img), cuda(snd), None)
        old_i, old_g = host(d["image_feat"], d["sound_feat_positive"])
        old_i2, = host(m(cuda(img2), None, None)["image_feat"])
    r = var_amd.IntrinsicReward(m).capture(B)
    i, g, w = host(*r.step(cuda(img), cuda(snd)))
    i2, g2, w2 = host(*r.step(cuda(img2)))
    print(f"B={B}: new vs old image_feat {np.abs(i - old_i).max():.2e} goal_feat {np.abs(g - old_g).max():.2e} "
          f"image-only {np.abs(i2 - old_i2).max():.2e}")
    np.testing.assert_allclose(i, old_i, atol=ATOL_PATHS, rtol=0)
    np.testing.assert_allclose(g, old_g, atol=ATOL_PATHS, rtol=0)
    np.testing.assert_allclose(i2, old_i2, atol=ATOL_PATHS, rtol=0)
    assert np.array_equal(g2, g)
    assert_reward_is_the_dot(i, g, w)
    assert_reward_is_the_dot(i2, g2, w2)


def test_two_launch_gru_with_fewer_clips_than_the_plan(var_amd, ref):
    """17 clips under a 64-env plan: the split-K product + gate kernel form (more than 16 clips) with nclips != the planned batch,
    where the slab strides follow the clips and the state slots the plan.  Same bounds as above."""
    m = hip_model(var_amd, ref)
    var_amd.IntrinsicReward(m).capture(64)                     # the context's reward plan is now 64 envs and only grows
    B = 17
    img, snd = rin.spread_inputs(B)
    snd[3] = 0.0
    want_i, want_g = rin.checker_image_feat(ref, img), rin.checker_goal_feat(ref, snd)
    with torch.no_grad():
        d = m(cuda(img), cuda(snd), None)
        old_i, old_g = host(d["image_feat"], d["sound_feat_positive"])
    r = var_amd.IntrinsicReward(m).capture(B)
    i, g, w = host(*r.step(cuda(img), cuda(snd)))
    print(f"B=17 under a 64 plan: goal_feat vs checker {np.abs(g - want_g).max():.2e}, vs training forward {np.abs(g - old_g).max():.2e}; "
          f"image_feat vs checker {np.abs(i - want_i).max():.2e}")
    np.testing.assert_allclose(g, want_g, atol=ATOL_CHECKER, rtol=0)
    np.testing.assert_allclose(i, want_i, atol=ATOL_CHECKER, rtol=0)
    np.testing.assert_allclose(g, old_g, atol=ATOL_PATHS, rtol=0)
    np.testing.assert_allclose(i, old_i, atol=ATOL_PATHS, rtol=0)
    assert_reward_is_the_dot(i, g, w)


# ---- 4 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,zero_clip,half_clip", [(1, 0, None), (1, None, 0), (8, 2, 5), (16, 15, 0)])
def test_fused_gru_step_with_silent_clips(var_amd, ref, B, zero_clip, half_clip):
    """At most 16 clips the GRU runs on the fused step kernel: one clip all-zero, one zero from frame 300 on."""
    m = hip_model(var_amd, ref)
    img, snd = rin.spread_inputs(B)
    if zero_clip is not None:
        snd[zero_clip] = 0.0
    if half_clip is not None:
        snd[half_clip, :, 300:] = 0.0
    want_g = rin.checker_goal_feat(ref, snd)
    with torch.no_grad():
        old_g, = host(m(None, cuda(snd), None)["sound_feat_positive"])      # the two-launch form
    r = var_amd.IntrinsicReward(m).capture(B)
    i, g, w = host(*r.step(cuda(img), cuda(snd)))
    print(f"B={B}: fused GRU goal_feat vs checker {np.abs(g - want_g).max():.2e}, vs two-launch form {np.abs(g - old_g).max():.2e}")
    np.testing.assert_allclose(g, want_g, atol=ATOL_CHECKER, rtol=0)
    np.testing.assert_allclose(g, old_g, atol=ATOL_PATHS, rtol=0)
    assert_reward_is_the_dot(i, g, w)


# ---- 5 ---------------------------------------------------------------------------------------------------------------
def test_200_replays_equal_eager_calls_bit_for_bit(var_amd, ref):
    from var_amd._lib import Context
    m = hip_model(var_amd, ref)
    B = 8
    r = var_amd.IntrinsicReward(m).capture(B)
    c = Context.get(0)
    flat = m.flat_parameters()
    gen = torch.Generator(device="cuda").manual_seed(77)
    e_i, e_g, e_w = outs(B)
    for k in range(200):
        img = torch.randint(0, 256, (B, 3, 96, 96), dtype=torch.uint8, device="cuda", generator=gen)
        with_goal = k % 2 == 0
        snd = None
        if with_goal:
            snd = torch.randn((B, 1, 600, 40), device="cuda", generator=gen) * 6.0
            snd[:, :, :, 0] += 18.0
            snd[k % B, :, 100 + k:] = 0.0
        else:
            e_g.copy_(r._goal_feat)
        i, g, w = r.step(img, snd)
        assert raw_step(c, flat, img, snd, B, e_i, e_g, e_w) == 0, c.lib.var_last_error(c.handle)
        torch.cuda.synchronize()
        assert torch.equal(i, e_i) and torch.equal(g, e_g) and torch.equal(w, e_w), f"replay {k} differs from the eager call"
        assert bool(torch.isfinite(w).all())


# ---- 6 ---------------------------------------------------------------------------------------------------------------
def test_u8_equals_f32_and_strided_batch(var_amd, ref):
    from var_amd._lib import Context
    m = hip_model(var_amd, ref)
    B = 8
    r = var_amd.IntrinsicReward(m).capture(B)
    c = Context.get(0)
    flat = m.flat_parameters()
    img, snd = rin.spread_inputs(B)
    img_f32 = cuda(img.astype(np.float32) / np.float32(255.0))      # (IEEE division on the host, as the kernel divides)
    img, snd = cuda(img), cuda(snd)
    a = outs(B)
    assert raw_step(c, flat, img, snd, B, *a) == 0
    b = outs(B)
    assert raw_step(c, flat, img_f32, snd, B, *b) == 0
    wide = torch.zeros((B, 4, 96, 96), dtype=torch.uint8, device="cuda")
    wide[:, 3] = 201                                            # (a fourth plane the kernel must not read)
    wide[:, :3] = img
    s = outs(B)
    assert raw_step(c, flat, wide, snd, B, *s) == 0 and wide.stride(0) == 4 * 96 * 96
    torch.cuda.synchronize()
    for x, y, z in zip(a, b, s):
        assert torch.equal(x, y), "u8 and f32 / 255 inputs differ"
        assert torch.equal(x, z), "a strided batch differs"


# ---- 7 ---------------------------------------------------------------------------------------------------------------
def test_weights_are_frozen_at_capture_and_follow_a_recapture(var_amd, ref):
    m = hip_model(var_amd, ref)
    B = 8
    r = var_amd.IntrinsicReward(m).capture(B)
    img, snd = rin.spread_inputs(B)
    i0, g0, w0 = host(*r.step(cuda(img), cuda(snd)))
    second = rin.spread_checker(head_seed=6)
    with torch.no_grad():
        second.imgBranch[0].weight.mul_(1.1)
        second.cnn[0].bias.add_(0.05)
    arena = m.flat_parameters().data_ptr()
    m.load_state_dict(second.state_dict())
    assert m.flat_parameters().data_ptr() == arena              # (loaded in place: the graphs' params pointer still holds)
    i1, g1, w1 = host(*r.step(cuda(img), cuda(snd)))            # no re-capture: the weights of the first capture
    assert np.array_equal(i1, i0) and np.array_equal(g1, g0) and np.array_equal(w1, w0)
    r.capture(B)
    i2, g2, w2 = host(*r.step(cuda(img), cuda(snd)))
    want_i, want_g = rin.checker_image_feat(second, img), rin.checker_goal_feat(second, snd)
    assert np.abs(want_i - i0).max() > 1e-2 and np.abs(want_g - g0).max() > 1e-2      # (the two checkpoints do differ)
    np.testing.assert_allclose(i2, want_i, atol=ATOL_CHECKER, rtol=0)
    np.testing.assert_allclose(g2, want_g, atol=ATOL_CHECKER, rtol=0)
    assert_reward_is_the_dot(i2, g2, w2)


# ---- 8 ---------------------------------------------------------------------------------------------------------------
def test_training_step_and_policy_on_the_same_context_leave_the_graphs_alone(var_amd, ref):
    from var_amd._lib import Context
    m = hip_model(var_amd, ref)
    B = 8
    r = var_amd.IntrinsicReward(m).capture(B)
    c = Context.get(0)
    img, snd = rin.spread_inputs(B)
    img2 = rin.spread_images(B, 31)
    i0, g0, w0 = host(*r.step(cuda(img), cuda(snd)))
    j0, _, v0 = host(*r.step(cuda(img2)))
    # an iTHOR training step at batch 32 in bf16 mode: re-plans the training workspace, flips the context's switches
    torch.manual_seed(3)
    tm = var_amd.IthorVARPretextNet(cfg()).to("cuda").set_precision("bf16")
    tr = var_amd.IthorTrainer(tm)
    timg, tsnd = rin.spread_inputs(32, 41)
    tr.step(cuda(timg), cuda(tsnd), cuda(tsnd[::-1].copy()))
    torch.cuda.synchronize()
    left = (c.lib.var_ithor_set_bf16(c.handle, -1), c.lib.var_ithor_set_gru_sequence(c.handle, -1),
            c.lib.var_ithor_saved_generation(c.handle))
    assert left[0] == 1                                        # (the training model's bf16 mode is what the context holds)
    torch.manual_seed(4)
    pol = var_amd.IthorNetPolicy(None, rin.Discrete(8), config=rin.POLICY_CFG, base='ai2thor_VAR', base_kwargs=rin.POLICY_KW).to("cuda")
    obs, hxs, masks = rin.policy_batch(16, 9)
    with torch.no_grad():
        pol.act(obs, hxs, masks, deterministic=True)
    torch.cuda.synchronize()
    j1, g1, v1 = host(*r.step(cuda(img2)))
    assert np.array_equal(j1, j0) and np.array_equal(g1, g0) and np.array_equal(v1, v0)
    i1, g1, w1 = host(*r.step(cuda(img), cuda(snd)))
    assert np.array_equal(i1, i0) and np.array_equal(g1, g0) and np.array_equal(w1, w0)
    assert (c.lib.var_ithor_set_bf16(c.handle, -1), c.lib.var_ithor_set_gru_sequence(c.handle, -1),
            c.lib.var_ithor_saved_generation(c.handle)) == left


# ---- 9 ---------------------------------------------------------------------------------------------------------------
def test_error_paths_leave_the_outputs_untouched(var_amd, ref):
    from var_amd._lib import Context, current_stream_handle, ptr
    ERR_ARG, ERR_PLAN, ERR_STATE = -1, -3, -4
    m = hip_model(var_amd, ref)
    flat = m.flat_parameters()
    B = 8
    img, snd = rin.spread_inputs(B)
    img, snd = cuda(img), cuda(snd)
    c = Context(0)                                              # a context of its own: nothing planned yet
    try:
        o = outs(B, 7.0)

        def untouched():
            torch.cuda.synchronize()
            return all(bool((t == 7.0).all()) for t in o)

        assert raw_step(c, flat, img, snd, B, *o) == ERR_PLAN and untouched()          # before the plan
        assert c.lib.var_ithor_reward_pack(c.handle, current_stream_handle(), ptr(flat)) == ERR_PLAN
        assert c.lib.var_ithor_reward_plan(c.handle, B, 84) == ERR_ARG
        assert b"96" in c.lib.var_last_error(c.handle)
        assert c.lib.var_ithor_reward_plan(c.handle, 65, 96) == ERR_ARG
        assert c.lib.var_ithor_reward_plan(c.handle, 0, 96) == ERR_ARG
        assert raw_step(c, flat, img, snd, B, *o) == ERR_PLAN and untouched()          # (the refused plans planned nothing)
        assert c.lib.var_ithor_reward_plan(c.handle, B, 96) == 0
        assert raw_step(c, flat, img, snd, B, *o) == ERR_STATE and untouched()         # before the pack
        assert b"pack" in c.lib.var_last_error(c.handle)
        assert c.lib.var_ithor_reward_pack(c.handle, current_stream_handle(), None) == ERR_ARG
        assert c.lib.var_ithor_reward_pack(c.handle, current_stream_handle(), ptr(flat)) == 0
        big = outs(B + 1, 7.0)
        img9 = torch.zeros((B + 1, 3, 96, 96), dtype=torch.uint8, device="cuda")
        assert raw_step(c, flat, img9, None, B + 1, *big) == ERR_PLAN                  # B over the plan
        torch.cuda.synchronize()
        assert all(bool((t == 7.0).all()) for t in big)
        assert raw_step(c, flat, None, snd, B, *o) == ERR_ARG and untouched()          # NULL image
        assert raw_step(c, flat, img, snd, B, o[0], None, o[2]) == ERR_ARG and untouched()      # NULL goal_feat
        assert raw_step(c, flat, img, snd, B, *o, bstride=IMG_FLOATS - 1) == ERR_ARG and untouched()
        assert raw_step(c, flat, img, snd, 0, *o) == ERR_ARG and untouched()
        other = flat.clone()
        assert raw_step(c, other, img, snd, B, *o) == ERR_STATE and untouched()        # not the packed arena
        assert raw_step(c, flat, img, snd, B, *o) == 0 and not untouched()             # and the good call does run
    finally:
        torch.cuda.synchronize()
        c.lib.var_destroy(c.handle)
        c.handle = None
    r = var_amd.IntrinsicReward(m).capture(B)
    with pytest.raises(var_amd.VarHipError):
        r.step(img)                                             # image-only before any goal step
    with pytest.raises(var_amd.VarHipError):
        r.step(img.cpu(), snd)
    with pytest.raises(var_amd.VarHipError):
        r.step(img, snd.cpu())
    with pytest.raises(var_amd.VarHipError):
        r.step(img, torch.zeros((B, 1, 100, 40), device="cuda"))
    with pytest.raises(var_amd.VarHipError):
        var_amd.IntrinsicReward(m).capture(65)
    with pytest.raises(var_amd.VarHipError):
        r.step(img)                                             # (the refused steps cached nothing)
    r.step(img, snd)
    r.step(img)
    torch.cuda.synchronize()

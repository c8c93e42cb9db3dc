"""Host logic of the RL-stage helper: streaming return normalisation against the fixture made with
the reference's RunningMeanStd, and (GPU) the intrinsic reward through the frozen HIP encoder."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_return_normalizer_matches_reference_stream(golden_dir):
    import var_amd
    fx = dict(np.load(os.path.join(golden_dir, "reward_norm.npz")))
    norm = var_amd.ReturnNormalizer(num_envs=fx["rews"].shape[1])
    out = np.stack([norm(fx["rews"][t], fx["news"][t]) for t in range(fx["rews"].shape[0])])
    assert np.array_equal(out, fx["out"])                         # same float64 arithmetic, same order
    assert norm.ret_rms.mean == fx["mean"] and norm.ret_rms.var == fx["var"] and norm.ret_rms.count == fx["count"]
    norm2 = var_amd.ReturnNormalizer(num_envs=fx["rews"].shape[1], cliprew=1.5)
    out2 = np.stack([norm2(fx["rews"][t], fx["news"][t]) for t in range(fx["rews"].shape[0])])
    assert np.array_equal(out2, fx["out_clip15"]) and np.max(np.abs(out2)) == 1.5 and np.mean(np.abs(out2) == 1.5) > 0.01


def test_running_mean_std_equals_batch_statistics():
    import var_amd
    rng = np.random.default_rng(0)
    x = rng.normal(2.0, 3.0, size=(1000, 4))
    rms = var_amd.RunningMeanStd(shape=(4,), epsilon=1e-12)
    for chunk in np.split(x, 10):
        rms.update(chunk)
    assert np.allclose(rms.mean, x.mean(0), atol=1e-9) and np.allclose(rms.var, x.var(0), atol=1e-9)


@pytest.mark.gpu
def test_intrinsic_reward_on_hip_encoder(golden_dir):
    """getEmbeddings + calcReward of the reference wrapper on the HIP forward at the RL batch (8 envs), incl. the
    cached-goal-sound protocol; expected values are the reference's own forward outputs (kuka_edge.npz)."""
    import torch
    import var_amd
    sd = dict(np.load(os.path.join(golden_dir, "kuka_weights.npz")))
    fx = dict(np.load(os.path.join(golden_dir, "kuka_edge.npz")))
    cfg = types.SimpleNamespace(img_dim=(3, 84, 84), sound_dim=(1, 100, 40), representationDim=3)
    m = var_amd.VARPretextNet(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    m = m.to("cuda")
    r = var_amd.IntrinsicReward(m)
    img, goal = fx["image"], fx["sound_positive"]
    image_feat, goal_feat, _ = r.embeddings(img, goal)
    env_rew = np.linspace(-1, 1, img.shape[0])
    total, dot, ss = r.reward(env_rew, image_feat, goal_feat)
    assert np.max(np.abs(dot - fx["d.reward"])) < 1e-4 and np.all(ss == 0)
    assert np.max(np.abs(total - (fx["d.reward"] + env_rew))) < 1e-4
    # later steps of the episode: the goal sound is not embedded again
    image_feat2, goal_feat2, _ = r.embeddings(img, None)
    assert np.array_equal(goal_feat2, goal_feat) and np.array_equal(image_feat2, image_feat)
    # the graph-captured latency path gives the same numbers (the image branch through the small-batch kernels,
    # include/var_hip.h: save_for_bwd = 2 -- equal within rounding; the sound branch bit for bit)
    r.capture(img.shape[0])
    f1, g1, dot1 = r.step(torch.from_numpy(img).cuda(), torch.from_numpy(goal).cuda())
    assert np.max(np.abs(f1.cpu().numpy() - image_feat)) < 1e-6 and np.array_equal(g1.cpu().numpy(), goal_feat)
    assert np.max(np.abs(dot1.cpu().numpy() - fx["d.reward"])) < 1e-4
    f2, g2, dot2 = r.step(torch.from_numpy(img).cuda(), None)
    assert np.array_equal(f2.cpu().numpy(), f1.cpu().numpy()) and np.array_equal(g2.cpu().numpy(), goal_feat)
    # (round 4: in that graph the image head's launch finishes the embeddings and takes the row dot itself, var_set_reward_dot:
    # same sums as heads_finish_kernel + row_dot_kernel)
    assert np.array_equal(dot2.cpu().numpy(), dot1.cpu().numpy())


def _kuka_model(golden_dir, hw):
    """The fixture weights on the GPU at either image size (the image head's 64 x 3 x 3 input is the same at 84 and 96)."""
    import torch
    import var_amd
    sd = dict(np.load(os.path.join(golden_dir, "kuka_weights.npz")))
    cfg = types.SimpleNamespace(img_dim=(3, hw, hw), sound_dim=(1, 100, 40), representationDim=3)
    m = var_amd.VARPretextNet(cfg)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return m.to("cuda")


@pytest.mark.gpu
@pytest.mark.parametrize("hw,B", [(84, 8), (84, 32), (96, 8)])
def test_image_only_reward_step_is_its_own_dot(golden_dir, hw, B):
    """The image-only graph of IntrinsicReward returns <image_feat, goal_feat> of ITS OWN step at every size, whether the dot
    rides in the image-head launch (84 x 84, B <= 16) or is a launch of its own after the embeddings (96 x 96, more rows)."""
    import torch
    import var_amd
    r = var_amd.IntrinsicReward(_kuka_model(golden_dir, hw)).capture(B)
    rng = np.random.default_rng(hw + B)
    img1, img2 = (torch.from_numpy(rng.integers(0, 256, size=(B, 3, hw, hw), dtype=np.uint8)).cuda() for _ in range(2))
    goal = torch.from_numpy(rng.standard_normal((B, 1, 100, 40)).astype(np.float32)).cuda()
    _, _, dot1 = r.step(img1, goal)
    dot1 = dot1.cpu().numpy().copy()
    f2, g2, dot2 = r.step(img2, None)
    f2, g2, dot2 = f2.cpu().numpy(), g2.cpu().numpy(), dot2.cpu().numpy()
    want = np.sum(f2 * g2, 1)
    assert np.max(np.abs(dot2 - want)) < 1e-6, (dot2, want)
    assert not np.array_equal(dot2, dot1)                  # (different images: not the with-goal step's value)


@pytest.mark.gpu
def test_reward_dot_is_disarmed_by_its_forward(golden_dir):
    """var_set_reward_dot arms ONE var_arm_encoder_fwd, whichever kernels that forward ran: a later unarmed forward -- here
    one that takes the in-launch dot path -- writes nothing through the old pointer."""
    import torch
    from var_amd._lib import Context, current_stream_handle, ptr
    c = Context.get(0)
    B = 8
    goal = torch.randn(B, 3, device="cuda")
    X = torch.zeros(B, device="cuda")

    def forward(hw):
        m = _kuka_model(golden_dir, hw)
        flat = m.flat_parameters()
        c.ensure_plan(B, hw)
        m.hip_weights(c, force=True)
        img = torch.from_numpy(np.random.default_rng(hw).integers(0, 256, size=(B, 3, hw, hw), dtype=np.uint8)).cuda()
        feat = torch.empty(B, 3, device="cuda")
        c.check(c.lib.var_arm_encoder_fwd(c.handle, current_stream_handle(), ptr(flat), ptr(img), 1, img.stride(0), None, None,
                                          B, hw, ptr(feat), None, None, None, None, 2), "var_arm_encoder_fwd")
        torch.cuda.synchronize()

    c.check(c.lib.var_set_reward_dot(c.handle, ptr(goal), ptr(X)), "var_set_reward_dot")
    forward(96)                                            # armed: the dot is a launch of its own at 96 x 96
    X.fill_(-12345.0)
    torch.cuda.synchronize()
    forward(84)                                            # unarmed: 84 x 84, B = 8 would take the in-launch dot
    assert torch.all(X == -12345.0), X


@pytest.mark.gpu
def test_row_dot_is_calc_reward_and_rejects_bad_arguments():
    """var_row_dot = calcReward's torch.sum(a * b, dim=1) (vec_pretext_normalize.py:96-101) in one launch."""
    import torch
    import var_amd
    from var_amd._lib import Context, VarHipError, current_stream_handle, ptr
    c = Context.get(0)
    g = torch.Generator().manual_seed(3)
    for rows, dim in ((8, 3), (300, 3), (5, 64)):
        a, b = torch.randn(rows, dim, generator=g).cuda(), torch.randn(rows, dim, generator=g).cuda()
        out = torch.empty(rows, device="cuda")
        c.check(c.lib.var_row_dot(c.handle, current_stream_handle(), ptr(a), ptr(b), rows, dim, ptr(out)), "var_row_dot")
        want = (a.double() * b.double()).sum(1)
        np.testing.assert_allclose(out.cpu().numpy(), want.cpu().numpy(), rtol=0, atol=1e-6 * dim)
    with pytest.raises(VarHipError):
        c.check(c.lib.var_row_dot(c.handle, current_stream_handle(), ptr(a), ptr(b), 5, 65, ptr(out)), "var_row_dot")
    with pytest.raises(VarHipError):
        c.check(c.lib.var_row_dot(c.handle, current_stream_handle(), None, ptr(b), 5, 3, ptr(out)), "var_row_dot")

"""Host-side checks of the PPO rollout restatement (tests/rollout_cpu.py) against the fixture made from the reference's
RolloutStorage and PPO (tests/golden/make_golden_rollout.py), of its closed-form loss gradients against torch autograd in
float64, and of the binding (no compute is called here)."""
import os
import types

import numpy as np
import pytest
import torch

from tests import rollout_cpu as rc

MODES = {"gae_proper": (True, True), "gae_free": (True, False), "plain_proper": (False, True), "plain_free": (False, False)}


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "rollout_t7.npz"))


def storage_from(gold):
    """The storage contents after the fixture's T inserts (storage.py:61-77), from what insert() was fed."""
    T, N = gold["in.reward"].shape[:2]
    one = np.ones((1, N, 1), np.float32)
    return dict(rewards=gold["in.reward"], value_preds=np.concatenate([gold["in.value"], np.zeros((1, N, 1), np.float32)]),
                masks=np.concatenate([one, gold["in.masks"]]), bad_masks=np.concatenate([one, gold["in.bad_masks"]]),
                next_value=gold["in.next_value"])


@pytest.mark.parametrize("mode", sorted(MODES))
def test_returns_restatement_is_bit_equal_to_the_reference(gold, mode):
    gae, proper = MODES[mode]
    s = storage_from(gold)
    assert set(np.unique(s["masks"])) == {0.0, 1.0} and set(np.unique(s["bad_masks"])) == {0.0, 1.0}
    ret, v = rc.compute_returns(s["rewards"], s["value_preds"], s["masks"], s["bad_masks"], s["next_value"], gae, rc.GAMMA, rc.LAMBDA,
                                proper)
    assert np.array_equal(ret.view(np.uint32), gold["ret." + mode].view(np.uint32))
    assert np.array_equal(v.view(np.uint32), gold["vp." + mode].view(np.uint32))


def test_advantages_restatement(gold):
    a = rc.advantages64(gold["ret.gae_proper"], gold["vp.gae_proper"])
    assert np.array_equal(rc.advantages_torch32(gold["ret.gae_proper"], gold["vp.gae_proper"]), gold["adv"])
    d = np.abs(gold["adv"] - a).max()
    print("torch fp32 advantages vs float64, fixture:", d, "; over 20 seeds at (7,5):", rc.advantage_distance(7, 5))
    assert d < 1e-6                                              # a few fp32 ulps of values below 4


def test_minibatch_restatement_equals_the_reference(gold):
    T, N = gold["in.reward"].shape[:2]
    s = storage_from(gold)
    z = lambda a: np.concatenate([np.zeros((1, *a.shape[1:]), a.dtype), a])             # noqa: E731  (slot 0 is never written)
    stores = {"obs.image": z(gold["in.image"]), "obs.pose": z(gold["in.pose"]), "actions": gold["in.actions"],
              "value_preds": gold["vp.gae_proper"], "returns": gold["ret.gae_proper"], "masks": s["masks"],
              "action_log_probs": gold["in.logp"], "advantages": gold["adv"]}
    mbs = rc.minibatches(stores, z(gold["in.hxs"]), gold["perm"], 2)
    assert [len(m["actions"]) for m in mbs] == [2 * T, 2 * T, T]                     # N = 5: two envs, two envs, one env
    # the reference yields the two full minibatches and raises on the short one (its loop indexes perm[5])
    assert int(gold["mb_count"]) == 2 and str(gold["mb_error"]) == "IndexError"
    for i in range(2):
        for k, v in mbs[i].items():
            assert np.array_equal(v, gold[f"mb{i}.{k}"]), (i, k)
    assert np.array_equal(mbs[2]["actions"], gold["in.actions"][:, gold["perm"][4]])


@pytest.mark.parametrize("kind", [0, 1])
def test_loss_restatement_against_the_reference_update(gold, kind):
    pre = f"loss{kind}."
    ls = gold[pre + "logstd"] if kind == 0 else None
    ref = rc.loss_ref(kind, gold[pre + "head"], ls, gold[pre + "value"], gold[pre + "action"], gold[pre + "old_logp"], gold[pre + "adv"],
                      gold[pre + "returns"], gold[pre + "value_preds"], 0.2, 0.5, 0.01, True)
    for k, v in ref.items():
        g = gold[pre + k].astype(np.float64).reshape(v.shape)
        # the fixture is fp32 torch on 35 rows: 1e-5 of the array's largest magnitude leaves two decimal orders over its rounding
        assert np.abs(g - v).max() <= 1e-5 * max(1.0, np.abs(v).max()), (k, np.abs(g - v).max())


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("kind, n", [(0, 1), (0, 4), (1, 1), (1, 8), (1, 16)])
@pytest.mark.parametrize("M", [1, 14, 257])
def test_closed_form_gradients_equal_autograd_in_float64(kind, n, M, clipped):
    d = rc.loss_inputs(kind, M, n, 100 * M + 10 * n + kind)
    ref = rc.loss_ref(kind, *rc.loss_args(d, clipped))
    t64 = rc.loss_torch(kind, *rc.loss_args(d, clipped), dtype=torch.float64)
    for k, v in ref.items():
        assert np.abs(t64[k].reshape(v.shape) - v).max() <= 1e-12, k


def test_closed_form_follows_autograd_at_the_kinks():
    """adv = 0, v == vp (l1 == l2 with the clip gate open), and a ratio of exactly 1: float64 autograd's answers."""
    d = rc.loss_inputs(1, 6, 4, 3)
    d["adv"][0] = 0.0
    d["value_preds"][1] = d["value"][1]
    d["old_logp"] = d["old_logp"].astype(np.float64)
    d["old_logp"][2, 0] = rc.logp64(1, d["head"], None, d["action"])[2]
    ref = rc.loss_ref(1, *rc.loss_args(d, True))
    t64 = rc.loss_torch(1, *rc.loss_args(d, True), dtype=torch.float64)
    for k, v in ref.items():
        assert np.abs(t64[k].reshape(v.shape) - v).max() <= 1e-12, k
    assert ref["g_value"][1, 0] == 0.5 * (np.float64(d["value"][1, 0]) - np.float64(d["returns"][1, 0])) / 6


def test_binding_and_shape_checks_without_compute():
    import var_amd
    from var_amd._lib import MoveSeg, EXPORTED_SYMBOLS
    lib = var_amd.load_library()
    for name in ("var_rollout_move", "var_rollout_returns", "var_ppo_head"):
        assert name in EXPORTED_SYMBOLS and hasattr(lib, name)
    import ctypes
    assert ctypes.sizeof(MoveSeg) == 64                          # var_move_seg: two pointers and six longs
    assert {"RolloutStorage", "PPO", "ppo_loss"} <= set(dir(var_amd))

    class Discrete:
        n = 4
    cfg = types.SimpleNamespace(RLObsIgnore=[])
    with pytest.raises(var_amd.VarHipError):
        var_amd.RolloutStorage(4, 2, {'pose': (2,)}, Discrete(), 8, cfg, device="cpu")
    with pytest.raises(var_amd.VarHipError):
        var_amd.ppo_loss(torch.zeros(3, 4), None, torch.zeros(3, 1), torch.zeros(3, 1, dtype=torch.int64), torch.zeros(3, 1),
                         torch.zeros(3, 1), torch.zeros(3, 1), torch.zeros(3, 1), kind=1, clip_param=0.2, value_loss_coef=0.5,
                         entropy_coef=0.01)

    class Stub(torch.nn.Module):
        is_recurrent = False
    with pytest.raises(NotImplementedError):
        var_amd.PPO(Stub(), 0.2, 1, 1, 0.5, 0.01, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    pol = types.SimpleNamespace()
    from var_amd.actor_critic import _ArenaPolicy
    with pytest.raises(NotImplementedError, match="var_amd.PPO"):
        _ArenaPolicy.evaluate_actions(pol, None, None, None, None)

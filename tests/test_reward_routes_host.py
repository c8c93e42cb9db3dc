"""The reward step's routes (var_amd/reward_step.py): which C entry runs for which kind of step, in which order, and which of
its pointer arguments are NULL -- RewardStep.launch driven by a context that records the calls, over CPU tensors.  The
expected table is written out below, one row per (encoder, sound_sound, clip table, with_goal, with_cur).  No GPU."""
import types

import pytest
import torch

B, HW = 8, 84
OPERANDS = ("image", "goal", "cur", "image_feat", "goal_feat", "cur_feat", "reward", "reward_img", "reward_snd")
NO_STREAM = ("var_set_reward_dot",)                              # (every other entry takes the stream behind the handle)


class Lib:
    """Every entry exists, records (name, args) and returns 0 -- or what `returns` says."""

    def __init__(self, returns):
        self.calls, self.returns = [], returns

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.returns.get(name, 0)
        return entry


class Ctx:
    handle = "handle"

    def __init__(self, returns):
        self.lib, self.plans = Lib(returns), []

    def stream(self):
        return None

    def check(self, rc, what):
        assert rc == 0, what

    def ensure_plan(self, batch, hw):
        self.plans.append((batch, hw))


def build(encoder, sound_sound, with_table):
    """-> (RewardStep over CPU tensors, its recording context, {address: operand name})"""
    from var_amd.ithor import IthorVARPretextNet
    from var_amd.reward_step import RewardStep
    flat = torch.zeros(16)
    c = Ctx({"var_ithor_param_count": flat.numel()})
    config = types.SimpleNamespace(img_dim=(3, HW, HW), sound_dim=(1, 4, 4))
    if encoder == "ithor":
        class Encoder(IthorVARPretextNet):                       # (isinstance is what tells the encoders apart)
            def __init__(self):
                pass
        model = Encoder()
        model.__dict__.update(config=config, flat_parameters=lambda: flat)
    else:
        weights = types.SimpleNamespace(bind=lambda: c.lib.calls.append(("bind", ())))
        packs = []
        model = types.SimpleNamespace(config=config, flat_parameters=lambda: flat, packs=packs,
                                      hip_weights=lambda ctx, force=False: packs.append((ctx, force)) or weights)
    table = types.SimpleNamespace(feat=torch.zeros(6, 3), rows=5, silent=5, checked=[])
    table.check = lambda m, f=None: table.checked.append((m, f))
    t = {"image": torch.zeros(B, 3, HW, HW, dtype=torch.uint8), "image_feat": torch.zeros(B, 3), "goal_feat": torch.zeros(B, 3),
         "reward": torch.zeros(B)}
    if with_table:
        t.update(goal=torch.zeros(B, dtype=torch.int32), cur=torch.zeros(B, dtype=torch.int32))
    else:
        t["goal"] = torch.zeros(B, 1, 4, 4)
        if sound_sound:
            t["cur"] = torch.zeros(B, 1, 4, 4)
    if sound_sound:
        t.update(cur_feat=torch.zeros(B, 3), reward_img=torch.zeros(B), reward_snd=torch.zeros(B))
    rs = RewardStep(c, model, B, is_u8=True, sound_sound=sound_sound, clip_table=table if with_table else None, **t)
    assert table.checked == ([(model, flat)] if with_table else [])
    names = {v.data_ptr(): k for k, v in t.items()}
    names.update({flat.data_ptr(): "flat", table.feat.data_ptr(): "table"})
    assert len(names) == len(t) + 2 and set(t) <= set(OPERANDS)
    return rs, c, names, model


def rendered(c, names, since=0):
    """The recorded calls as 'entry(pointer arguments in order, - for NULL)'; scalars are left out."""
    out = []
    for name, args in c.lib.calls[since:]:
        if name == "bind":
            out.append("bind")
            continue
        assert args[0] == "handle"
        if name not in NO_STREAM:
            assert args[1] is None                               # the context's stream
        ptrs = [("-" if a is None else names[a]) for a in args[1 if name in NO_STREAM else 2:] if a is None or a in names]
        if name == "var_arm_encoder_fwd":
            assert args[-1] == 2 and args[8:10] == (B, HW)       # save_for_bwd stays 2
        out.append(f"{name}({' '.join(ptrs)})")
    return out


# ---- the table ---------------------------------------------------------------------------------------------------------------
IMAGE_ONLY_FWD = "var_arm_encoder_fwd(flat image - - image_feat - - - -)"
ARM_GOAL = ["bind", "var_arm_encoder_fwd(flat image goal - image_feat goal_feat - - -)", "var_row_dot(image_feat goal_feat reward)"]
ARM_CACHED = ["bind", "var_set_reward_dot(goal_feat reward)", IMAGE_ONLY_FWD]
ARM_DOTS = "var_reward_dots(image_feat goal_feat cur_feat reward reward_img reward_snd)"
ARM_SS_GOAL = ["bind", "var_arm_encoder_fwd(flat image goal cur image_feat goal_feat cur_feat - -)", ARM_DOTS]
ARM_SS_CACHED = ["bind", "var_arm_encoder_fwd(flat image - cur image_feat - cur_feat - -)", ARM_DOTS]
ARM_IDS = ["bind", IMAGE_ONLY_FWD, "var_reward_dots_ids(image_feat table goal - goal_feat - reward - -)"]
ARM_IDS_CUR = ["bind", IMAGE_ONLY_FWD, "var_reward_dots_ids(image_feat table goal cur goal_feat cur_feat reward reward_img reward_snd)"]
ITHOR_GOAL = ["var_ithor_reward_step_ex(flat image goal - image_feat goal_feat - reward - -)"]
ITHOR_CACHED = ["var_ithor_reward_step_ex(flat image - - image_feat goal_feat - reward - -)"]
ITHOR_SS_GOAL = ["var_ithor_reward_step_ex(flat image goal cur image_feat goal_feat cur_feat reward reward_img reward_snd)"]
ITHOR_SS_CACHED = ["var_ithor_reward_step_ex(flat image - cur image_feat goal_feat cur_feat reward reward_img reward_snd)"]
ITHOR_IDS = ["var_ithor_reward_step_ids(flat image table goal - image_feat goal_feat - reward - -)"]
ITHOR_IDS_CUR = ["var_ithor_reward_step_ids(flat image table goal cur image_feat goal_feat cur_feat reward reward_img reward_snd)"]

# (encoder, sound_sound, clip table) -> the entries of launch(True, sound_sound), launch(False, sound_sound), launch(True, False)
ROUTES = {
    ("arm", False, False): (ARM_GOAL, ARM_CACHED, ARM_GOAL),
    ("arm", True, False): (ARM_SS_GOAL, ARM_SS_CACHED, ARM_GOAL),
    ("arm", False, True): (ARM_IDS, ARM_IDS, ARM_IDS),
    ("arm", True, True): (ARM_IDS_CUR, ARM_IDS_CUR, ARM_IDS),
    ("ithor", False, False): (ITHOR_GOAL, ITHOR_CACHED, ITHOR_GOAL),
    ("ithor", True, False): (ITHOR_SS_GOAL, ITHOR_SS_CACHED, ITHOR_GOAL),
    ("ithor", False, True): (ITHOR_IDS, ITHOR_IDS, ITHOR_IDS),
    ("ithor", True, True): (ITHOR_IDS_CUR, ITHOR_IDS_CUR, ITHOR_IDS),
}


@pytest.mark.parametrize("route", list(ROUTES), ids=lambda r: f"{r[0]}-{'ss' if r[1] else 'plain'}-{'table' if r[2] else 'sounds'}")
def test_every_route_makes_its_calls_in_order_with_its_nulls(route):
    encoder, ss, with_table = route
    rs, c, names, _ = build(*route)
    for (with_goal, with_cur), want in zip(((True, ss), (False, ss), (True, False)), ROUTES[route]):
        since = len(c.lib.calls)
        assert rs.launch(with_goal, with_cur) is None
        assert rendered(c, names, since) == want, (route, with_goal, with_cur)


@pytest.mark.parametrize("route", list(ROUTES), ids=str)
def test_the_plan_carries_the_flag_iff_sound_sound_and_no_table(route):
    encoder, ss, with_table = route
    rs, c, names, model = build(*route)
    if encoder == "arm":                                         # the Kuka plan has no flags: var_plan for the batch, weights packed
        assert c.plans == [(B, HW)] and model.packs == [(c, True)] and c.lib.calls == []
        return
    assert [name for name, _ in c.lib.calls] == ["var_ithor_param_count", "var_ithor_reward_plan_ex", "var_ithor_reward_pack"]
    assert c.lib.calls[1][1] == ("handle", B, HW, int(ss and not with_table))        # VAR_IREW_SOUND_SOUND == 1
    assert rendered(c, names, 2) == ["var_ithor_reward_pack(flat)"] and c.plans == []


def test_a_plain_arm_step_never_leaves_a_stale_dot_armed():
    """var_set_reward_dot arms the NEXT forward; var_row_dot reads what the forward wrote.  A step without a goal must not run
    the row dot, a step with one must not arm the forward."""
    for ss in (False, True):
        rs, c, names, _ = build("arm", ss, False)
        rs.launch(False, False)
        entries = [name for name, _ in c.lib.calls]
        assert "var_row_dot" not in entries and entries.index("var_set_reward_dot") < entries.index("var_arm_encoder_fwd")
        since = len(c.lib.calls)
        rs.launch(True, False)
        assert "var_set_reward_dot" not in [name for name, _ in c.lib.calls[since:]]


def test_a_kept_goal_needs_a_cached_one():
    import numpy as np
    import var_amd
    rs, _, _, _ = build("ithor", True, True)
    with pytest.raises(var_amd.VarHipError, match=r"CollectStep.observe: no goal embedding is cached yet for envs \[0, 2\] -- reset\(\)"):
        rs.kept_goals(np.array([-1, 3, -1, 5, 0, 0, 0, 0], np.int32), "CollectStep.observe", "reset() or pass their goal ids")
    kept = rs.kept_goals(np.arange(B, dtype=np.int32), "IntrinsicReward.step_ids", "pass their goal ids")
    assert not kept.any() and not rs.goal_set.any()              # (the caller commits after the replay)
    rs.goal_set |= ~kept
    assert rs.kept_goals(np.full(B, -1, np.int32), "x", "y").all()

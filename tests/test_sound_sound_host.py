"""Host side of the sound-sound reward term (config.RLRewardSoundSound): the numpy restatement of var_reward_dots
(tests/sound_sound_cpu.py) is pinned to IntrinsicReward.reward -- calcReward's own arithmetic -- bit for bit, the groupings it
must not be confused with are shown to differ, and the new entries are declared, exported and bound.  No GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import sound_sound_cpu as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS = 20000


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def host_reward(sound_sound):
    import var_amd
    return var_amd.IntrinsicReward(types.SimpleNamespace(eval=lambda: None), sound_sound=sound_sound)


def test_restatement_equals_calc_reward_bit_for_bit():
    img, goal, cur = ss.unit_rows(ROWS, 3, seed=11)
    env = np.random.default_rng(12).normal(0, 1.5, ROWS)
    total, img_dot, snd_dot = host_reward(True).reward(env, img, goal, cur)
    out, a, b = ss.reward_dots(img, goal, cur)
    assert img_dot.dtype == snd_dot.dtype == np.float32 and total.dtype == np.float64
    assert np.array_equal(bits32(a), bits32(img_dot)) and np.array_equal(bits32(b), bits32(snd_dot))
    assert np.array_equal(bits64(out.astype(np.float64) + env), bits64(total))       # var_reward_norm_step's add
    # off: the first dot alone, var_row_dot's bits
    total0, img0, snd0 = host_reward(False).reward(env, img, goal)
    out0, a0, b0 = ss.reward_dots(img, goal, None)
    assert np.array_equal(bits32(out0), bits32(img0)) and np.array_equal(bits32(out0), bits32(ss.row_dot(img, goal)))
    assert not b0.any() and not snd0.any() and np.array_equal(bits64(out0.astype(np.float64) + env), bits64(total0))


def test_the_grouping_is_observable():
    """The check above cannot pass vacuously: one running sum over the six products, and the two dots added in float64, both
    differ from calcReward's grouping on seeded unit rows."""
    img, goal, cur = ss.unit_rows(ROWS, 3, seed=11)
    env = np.random.default_rng(12).normal(0, 1.5, ROWS)
    out, _, _ = ss.reward_dots(img, goal, cur)
    total = host_reward(True).reward(env, img, goal, cur)[0]
    one_sum = int((bits32(ss.single_sum(img, goal, cur)) != bits32(out)).sum())
    in_f64 = int((bits64(ss.dots_added_in_float64(img, goal, cur) + env) != bits64(total)).sum())
    print(f"rows of {ROWS} that differ: single six-term sum {one_sum}, dots added in float64 {in_f64}")
    assert one_sum >= 1 and in_f64 >= 1


def test_sound_sound_entries_are_declared_exported_and_bound():
    import var_amd
    from var_amd._lib import _SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "var_hip.h")).read()
    lib = ctypes.CDLL(var_amd.library_path())
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    want = {"var_reward_dots": (i, [vp, vp, vp, vp, vp, i, i, vp, vp, vp]),
            "var_ithor_reward_plan_ex": (i, [vp, i, i, i]),
            "var_ithor_reward_step_ex": (i, [vp, vp, vp, vp, i, l, vp, vp, i, vp, vp, vp, vp, vp, vp])}
    for name, sig in want.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(var_ctx\*", hdr), f"{name} is not declared in var_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert _SIGNATURES[name] == sig
    assert re.search(r"#define\s+VAR_IREW_SOUND_SOUND\s+1\b", hdr)


def test_collect_step_no_longer_refuses_the_mode_by_name():
    """CollectStep used to raise "RLRewardSoundSound is not provided" before looking at anything else; with a CPU model it
    now fails for the reason every CPU model fails."""
    import var_amd
    reward = var_amd.IntrinsicReward(types.SimpleNamespace(eval=lambda: None), sound_sound=True)
    with pytest.raises(var_amd.VarHipError) as e:
        var_amd.CollectStep(reward, None, None)
    assert "RLRewardSoundSound" not in str(e.value)

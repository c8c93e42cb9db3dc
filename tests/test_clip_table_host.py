"""Host side of the clip table (var_reward_dots_ids, var_ithor_reward_step_ids, var_ithor_reward_embed): the numpy restatement
of the id step (tests/clip_table_cpu.py) is pinned bit for bit to IntrinsicReward.reward -- calcReward's own arithmetic --
applied to the gathered rows, the mistakes it must not be confused with are shown to change the result, and the new entries
are declared, exported and bound.  No GPU."""
import ctypes
import os
import re
import types

import numpy as np
import pytest

from tests import clip_table_cpu as ct
from tests import sound_sound_cpu as ss

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROWS, TABLE = 20000, 257


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


def case():
    """20 000 seeded unit rows over a 257-row table, about a third of the goal ids -1."""
    rng = np.random.default_rng(31)
    img, cached, _ = ss.unit_rows(ROWS, 3, seed=11)
    table = ct.unit_table(TABLE, 3, seed=12)
    gid = rng.integers(0, TABLE, ROWS)
    gid[rng.random(ROWS) < 1 / 3] = -1
    cid = rng.integers(0, TABLE, ROWS)
    env = rng.normal(0, 1.5, ROWS)
    return img, cached, table, gid, cid, env


def host_reward(sound_sound):
    import var_amd
    return var_amd.IntrinsicReward(types.SimpleNamespace(eval=lambda: None), sound_sound=sound_sound)


def test_restatement_equals_calc_reward_on_the_gathered_rows_bit_for_bit():
    img, cached, table, gid, cid, env = case()
    assert 0.3 < (gid == -1).mean() < 0.37
    goal = np.where((gid >= 0)[:, None], table[np.maximum(gid, 0)], cached)
    got = ct.step_ids(img, table, gid, cid, cached)
    total, img_dot, snd_dot = host_reward(True).reward(env, img, goal, table[cid])
    assert np.array_equal(bits32(got["goal_feat"]), bits32(goal)) and np.array_equal(bits32(got["cur_feat"]), bits32(table[cid]))
    assert np.array_equal(bits32(got["out_img"]), bits32(img_dot)) and np.array_equal(bits32(got["out_snd"]), bits32(snd_dot))
    assert np.array_equal(bits64(got["out"].astype(np.float64) + env), bits64(total))
    assert not got["bad"].any()
    # no current ids: the first dot alone; no goal ids: every row keeps its cached embedding
    off = ct.step_ids(img, table, gid, None, cached)
    total0, img0, _ = host_reward(False).reward(env, img, goal)
    assert np.array_equal(bits32(off["out"]), bits32(img0)) and off["cur_feat"] is None and not off["out_snd"].any()
    assert np.array_equal(bits64(off["out"].astype(np.float64) + env), bits64(total0))
    kept = ct.step_ids(img, table, None, cid, cached)
    assert np.array_equal(bits32(kept["goal_feat"]), bits32(cached))
    assert np.array_equal(bits32(kept["out"]), bits32(ss.reward_dots(img, cached, table[cid])[0]))


def test_bad_ids_give_nan_rows_and_leave_the_cache():
    img, cached, table, gid, cid, _ = case()
    want = ct.step_ids(img, table, gid, cid, cached)
    for row, (g, c) in {5: (TABLE, 0), 6: (-2, 0), 7: (3, -1), 8: (-1, TABLE)}.items():
        g2, c2 = gid.copy(), cid.copy()
        g2[row], c2[row] = g, c
        got = ct.step_ids(img, table, g2, c2, cached)
        assert np.nonzero(got["bad"])[0].tolist() == [row]
        assert np.isnan(got["out"][row]) and np.isnan(got["out_img"][row]) and np.isnan(got["out_snd"][row])
        assert np.isnan(got["cur_feat"][row]).all() and np.array_equal(bits32(got["goal_feat"][row]), bits32(cached[row]))
        others = np.arange(ROWS) != row
        for k in ("out", "out_img", "out_snd", "goal_feat", "cur_feat"):
            assert np.array_equal(bits32(got[k][others]), bits32(want[k][others])), k


def test_each_injected_fault_is_observable():
    """The checks against this restatement cannot pass vacuously: each mistake changes the result on at least one row."""
    img, cached, table, gid, cid, env = case()
    want = ct.step_ids(img, table, gid, cid, cached)
    total = want["out"].astype(np.float64) + env
    counts = {}
    for fault in ct.FAULTS:
        got = ct.step_ids(img, table, gid, cid, cached, fault=fault)
        if fault == "dots_added_in_float64":
            assert got["out"].dtype == np.float64
            counts[fault] = int((bits64(got["out"] + env) != bits64(total)).sum())
        elif fault == "keep_overwrites":
            counts[fault] = int((bits32(got["goal_feat"]) != bits32(want["goal_feat"])).any(axis=1).sum())
        else:
            counts[fault] = int((bits32(got["out"]) != bits32(want["out"])).sum())
    print(f"rows of {ROWS} that differ: {counts}")
    assert all(n >= 1 for n in counts.values()), counts
    assert counts["keep_overwrites"] == (gid == -1).sum()       # every kept row lost its cached embedding


def test_clip_table_entries_are_declared_exported_and_bound():
    import var_amd
    from var_amd._lib import _SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "var_hip.h")).read()
    lib = ctypes.CDLL(var_amd.library_path())
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    want = {"var_reward_dots_ids": (i, [vp, vp, vp, vp, i, vp, vp, vp, vp, i, i, vp, vp, vp]),
            "var_ithor_reward_embed": (i, [vp, vp, vp, vp, i, vp]),
            "var_ithor_reward_step_ids": (i, [vp, vp, vp, vp, i, l, vp, i, vp, vp, i, vp, vp, vp, vp, vp, vp])}
    for name, sig in want.items():
        assert re.search(r"\bint\s+" + name + r"\s*\(var_ctx\*", hdr), f"{name} is not declared in var_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert _SIGNATURES[name] == sig
    assert var_amd.ClipTable.__name__ == "ClipTable"


def test_clip_table_refuses_bad_host_ids_and_a_cpu_model():
    import torch
    import var_amd
    table = var_amd.ClipTable.__new__(var_amd.ClipTable)
    table.rows = table.silent = 32
    ok = table.host_ids([0, 32, -1, 5], "goal_ids", 4, keep=True)
    assert ok.dtype == np.int32 and ok.tolist() == [0, 32, -1, 5]
    assert table.host_ids(torch.tensor([1, 2]), "current_ids", 2).tolist() == [1, 2]
    for ids, keep in (([0, 33], True), ([0, -2], True), ([0, -1], False), ([0.5, 1.0], True), ([1, 2, 3], True)):
        with pytest.raises(var_amd.VarHipError):
            table.host_ids(ids, "ids", 2, keep=keep)
    model = types.SimpleNamespace(flat_parameters=lambda: torch.zeros(4))
    model.eval = lambda: model
    with pytest.raises(var_amd.VarHipError, match="GPU"):
        var_amd.IntrinsicReward(model).build_clip_table(features=np.zeros((2, 1, 100, 40), np.float32))

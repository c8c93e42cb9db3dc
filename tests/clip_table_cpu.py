"""CPU restatement of the id step (include/var_hip.h: var_reward_dots_ids, the finishing thread of var_ithor_reward_step_ids):
the sound embeddings are rows of a clip table picked by per-row ids, then calcReward's sum in var_reward_dots' grouping --
tests/sound_sound_cpu.reward_dots, called unchanged.

    goal id g >= 0   goal[r] = table[g], and that becomes the row's cached embedding
    goal id g == -1  goal[r] = cached[r], untouched (no goal ids at all: every row)
    current id c     cur[r] = table[c]; no current ids: the first dot alone
    an id outside its range (goal < -1 or >= rows, current < 0 or >= rows): the row's outputs are NaN, cached[r] stays

`fault` selects one of the mistakes the kernels must NOT make; tests/test_clip_table_host.py shows each changes the result."""
import numpy as np

from tests import sound_sound_cpu as ss

FAULTS = ("keep_overwrites", "current_from_goal_id", "single_sum", "dots_added_in_float64")


def unit_table(rows, dim, seed):
    """Seeded float32 unit rows: a clip table as F.normalize leaves it."""
    return ss.unit_rows(rows, dim, seed)[0]


def step_ids(image_feat, table, goal_ids, cur_ids, cached, fault=None):
    """-> dict(out, out_img, out_snd, goal_feat (the cache afterwards), cur_feat | None).  goal_ids / cur_ids: int arrays | None."""
    image_feat, table = np.asarray(image_feat, np.float32), np.asarray(table, np.float32)
    rows, n = image_feat.shape[0], table.shape[0]
    gid = np.full(rows, -1, np.int64) if goal_ids is None else np.asarray(goal_ids, np.int64)
    cid = np.zeros(rows, np.int64) if cur_ids is None else np.asarray(cur_ids, np.int64)
    bad = (gid < -1) | (gid >= n) | (cid < 0) | (cid >= n)
    fresh = (gid >= 0) & ~bad
    if fault == "keep_overwrites":                               # -1 taken for a row of the table (the clamped one)
        fresh = ~bad
    g_row = np.where((gid >= 0) & (gid < n), gid, 0)             # the address is clamped, the value selected afterwards
    c_row = np.where((cid >= 0) & (cid < n), cid, 0)
    if fault == "current_from_goal_id":
        c_row = g_row
    goal = np.where(fresh[:, None], table[g_row], np.asarray(cached, np.float32)).astype(np.float32)
    cur = None if cur_ids is None else table[c_row].copy()
    if fault == "single_sum":
        out, (_, a, b) = ss.single_sum(image_feat, goal, cur), ss.reward_dots(image_feat, goal, cur)
    elif fault == "dots_added_in_float64":
        out, (_, a, b) = ss.dots_added_in_float64(image_feat, goal, cur), ss.reward_dots(image_feat, goal, cur)
    else:
        out, a, b = ss.reward_dots(image_feat, goal, cur)
    out, a, b = out.copy(), a.copy(), b.copy()
    out[bad], a[bad], b[bad] = np.nan, np.nan, np.nan
    if cur is not None:
        cur[bad] = np.nan
    return dict(out=out, out_img=a, out_snd=b, goal_feat=goal, cur_feat=cur, bad=bad)

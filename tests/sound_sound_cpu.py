"""CPU restatement of var_reward_dots (include/var_hip.h): calcReward's embedding reward with config.RLRewardSoundSound on
(Envs/vec_env/vec_pretext_normalize.py:96-101), in the kernel's own order of operations.

    a[r] = sum_k image_feat[r][k] * goal_feat[r][k]     k in index order, every product and every add rounded to float32
    b[r] = sum_k cur_feat[r][k] * goal_feat[r][k]       the same
    out[r] = a[r] + b[r]                                one float32 add

The float64 add of envReward is var_reward_norm_step's.  The two groupings below are what the kernel must NOT compute: they
differ from the reference on thousands of 20 000 unit rows, which is what makes the bit-for-bit checks mean something."""
import numpy as np


def unit_rows(rows, dim, seed):
    """Seeded float32 rows of unit length (what F.normalize leaves), three arrays: image, goal, current."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(3):
        x = rng.standard_normal((rows, dim)).astype(np.float32)
        out.append((x / np.maximum(np.sqrt((x * x).sum(axis=1, keepdims=True, dtype=np.float32)), np.float32(1e-12))).astype(np.float32))
    return out


def row_dot(a, b):
    """var_row_dot: the sum runs over k in index order in float32, no fused multiply-add."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    s = np.zeros(a.shape[0], np.float32)
    for k in range(a.shape[1]):
        s = (s + (a[:, k] * b[:, k]).astype(np.float32)).astype(np.float32)
    return s


def reward_dots(image_feat, goal_feat, cur_feat=None):
    """(out, out_img, out_snd) of var_reward_dots; cur_feat = None: out has var_row_dot's bits, out_snd is 0."""
    a = row_dot(image_feat, goal_feat)
    if cur_feat is None:
        return a, a, np.zeros_like(a)
    b = row_dot(cur_feat, goal_feat)
    return (a + b).astype(np.float32), a, b


def single_sum(image_feat, goal_feat, cur_feat):
    """Wrong: one running float32 sum over the 2 * dim products."""
    s = row_dot(image_feat, goal_feat)
    c, g = np.asarray(cur_feat, np.float32), np.asarray(goal_feat, np.float32)
    for k in range(c.shape[1]):
        s = (s + (c[:, k] * g[:, k]).astype(np.float32)).astype(np.float32)
    return s


def dots_added_in_float64(image_feat, goal_feat, cur_feat):
    """Wrong: the two float32 dots added in float64 (as if the second term joined envReward's add)."""
    return row_dot(image_feat, goal_feat).astype(np.float64) + row_dot(cur_feat, goal_feat).astype(np.float64)

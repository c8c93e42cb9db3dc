"""The frozen encoder's reward step as the C calls it is made of: the one place that says which entry runs for which kind of
step, which arguments are NULL and what is planned.  IntrinsicReward.capture and CollectStep own the buffers and the graphs;
both build a RewardStep over their buffers and capture launch().  tests/test_reward_routes_host.py holds the table below to
the calls, entry by entry.

    encoder  route                      entries, in order
    Kuka     plain, with a goal         var_arm_encoder_fwd (goal clip -> goal_feat), var_row_dot
    Kuka     plain, goal cached         var_set_reward_dot, var_arm_encoder_fwd (no sound: the forward itself leaves the dot)
    Kuka     sound-sound                var_arm_encoder_fwd (current clip as mfcc_neg -> cur_feat), var_reward_dots
    Kuka     clip table                 var_arm_encoder_fwd (image only), var_reward_dots_ids
    iTHOR    no table                   var_ithor_reward_step_ex (goal / current clip NULL where there is none)
    iTHOR    clip table                 var_ithor_reward_step_ids

launch(with_goal, with_cur): with_goal = this step embeds a new goal sound (ignored with a clip table: the goal ids say it per
env); with_cur = this step embeds the current sound, which counts only with sound_sound -- CollectStep's reset is
launch(True, False), every other step launch(with_goal, True).  Without the current sound its four arguments (clip or ids,
cur_feat, reward_img, reward_snd) are NULL and the step is the plain one.  var_weights_bind precedes every Kuka forward,
save_for_bwd is 2.  The iTHOR plan asks for VAR_IREW_SOUND_SOUND iff sound_sound and no table: only then a clip goes through
the sound branch beside the goal's."""
import numpy as np
import torch

from ._lib import VarHipError, ptr

VAR_IREW_SOUND_SOUND = 1


def prepare(c, model, flat, batch, flags=0):
    """What a reward step needs before its first launch: the iTHOR plan and the packed snapshot of the arena, or the Kuka plan
    and the model's own packed weight image (returned; None for iTHOR).  Plans only grow: earlier graphs stay valid."""
    from .ithor import IthorVARPretextNet
    hw = int(model.config.img_dim[1])
    if not isinstance(model, IthorVARPretextNet):
        c.ensure_plan(batch, hw)
        return model.hip_weights(c, force=True)                  # the frozen model's own packed image; the graphs keep its address
    if flat.numel() != c.lib.var_ithor_param_count():
        raise VarHipError("parameter arena does not match var_ithor_param_count()")
    c.check(c.lib.var_ithor_reward_plan_ex(c.handle, batch, hw, flags), "var_ithor_reward_plan_ex")
    c.check(c.lib.var_ithor_reward_pack(c.handle, c.stream(), ptr(flat)), "var_ithor_reward_pack")
    return None


class RewardStep:
    """One reward step over buffers the caller owns.  image (+ is_u8), image_feat, goal_feat (B,3), reward (B): always; goal /
    cur: the goal and current sound (B,) + sound_dim, or with clip_table the int32 goal / current ids (B); cur, cur_feat,
    reward_img, reward_snd: with sound_sound.  The callers refuse a model that is not on the GPU, each in its own words, before
    they allocate these; here the table is held to the model's arena, the plan made and the weights packed, once."""

    def __init__(self, c, model, batch, *, image, is_u8, goal, image_feat, goal_feat, reward, cur=None, cur_feat=None,
                 reward_img=None, reward_snd=None, sound_sound=False, clip_table=None):
        flat = model.flat_parameters()
        if clip_table is not None:
            clip_table.check(model, flat)
        self.c, self.flat, self.table, self.batch = c, flat, clip_table, int(batch)
        self.sound_sound = bool(sound_sound)
        self.hw = int(model.config.img_dim[1])
        self.weights = prepare(c, model, flat, self.batch, VAR_IREW_SOUND_SOUND if self.sound_sound and clip_table is None else 0)
        self.image, self.is_u8, self.goal, self.cur = image, int(is_u8), goal, cur
        self.image_feat, self.goal_feat, self.cur_feat = image_feat, goal_feat, cur_feat
        self.reward, self.reward_img, self.reward_snd = reward, reward_img, reward_snd
        self.goal_set = np.zeros(self.batch, bool)               # clip table, per env: has a goal embedding been cached?

    def launch(self, with_goal, with_cur):
        """Enqueue the route's C calls on the context's current stream; nothing else."""
        c, s, B, t = self.c, self.c.stream(), self.batch, self.table
        image = (ptr(self.flat), ptr(self.image), self.is_u8, self.image.stride(0))
        img_feat, goal_feat, reward = ptr(self.image_feat), ptr(self.goal_feat), ptr(self.reward)
        dim = int(self.image_feat.shape[1])
        on = bool(with_cur) and self.sound_sound
        cur, cur_feat, r_img, r_snd = [ptr(x) if on else None for x in (self.cur, self.cur_feat, self.reward_img, self.reward_snd)]
        goal = ptr(self.goal) if with_goal or t is not None else None
        if self.weights is None:                                 # iTHOR: one entry, 7 kernels with a table whatever the ids say
            if t is not None:
                c.check(c.lib.var_ithor_reward_step_ids(c.handle, s, *image, ptr(t.feat), t.rows + 1, goal, cur, B, img_feat,
                                                        goal_feat, cur_feat, reward, r_img, r_snd), "var_ithor_reward_step_ids")
            else:
                c.check(c.lib.var_ithor_reward_step_ex(c.handle, s, *image, goal, cur, B, img_feat, goal_feat, cur_feat, reward,
                                                       r_img, r_snd), "var_ithor_reward_step_ex")
            return
        self.weights.bind()

        def forward(goal, neg, goal_out, neg_out):               # 2: inference, small-batch kernels
            c.check(c.lib.var_arm_encoder_fwd(c.handle, s, *image, goal, neg, B, self.hw, img_feat, goal_out, neg_out, None, None,
                                              2), "var_arm_encoder_fwd")
        if t is not None:                                        # image only; the sounds' embeddings are gathered by the dots' launch
            forward(None, None, None, None)
            c.check(c.lib.var_reward_dots_ids(c.handle, s, img_feat, ptr(t.feat), t.rows + 1, goal, cur, goal_feat, cur_feat, B, dim,
                                              reward, r_img, r_snd), "var_reward_dots_ids")
        elif on:                                                 # the current sound is the forward's negative clip; no dot is armed
            forward(goal, cur, goal_feat if with_goal else None, cur_feat)
            c.check(c.lib.var_reward_dots(c.handle, s, img_feat, goal_feat, cur_feat, B, dim, reward, r_img, r_snd), "var_reward_dots")
        elif with_goal:                                          # calcReward's torch.sum(a * b, dim=1) as one launch
            forward(goal, None, goal_feat, None)
            c.check(c.lib.var_row_dot(c.handle, s, img_feat, goal_feat, B, dim, reward), "var_row_dot")
        else:                                                    # the goal embedding is cached: the forward itself leaves the dot
            c.check(c.lib.var_set_reward_dot(c.handle, goal_feat, reward), "var_set_reward_dot")
            forward(None, None, None, None)

    # ---- clip ids: the goal of each env ---------------------------------------------------------------------------------------
    def kept_goals(self, goal_ids, who, advice):
        """goal_ids as ClipTable.ids returned them -> kept (B,) bool: the envs that keep their cached goal (-1 in host ids; ids
        on the device are not read back, so none).  Raises for a kept env that has no goal yet.  After the replay the caller
        commits: goal_set |= ~kept."""
        kept = np.zeros(self.batch, bool) if torch.is_tensor(goal_ids) else goal_ids == -1
        if (kept & ~self.goal_set).any():
            raise VarHipError(f"{who}: no goal embedding is cached yet for envs "
                              f"{np.nonzero(kept & ~self.goal_set)[0].tolist()} -- {advice}")
        return kept

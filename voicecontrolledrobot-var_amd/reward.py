"""Frozen-encoder inference for the RL stage: embeddings, intrinsic reward and return-normalised reward
(BASELINE config 5).

Mirrors what the reference's vectorised-env wrapper does around the pretext model, without the simulator
plumbing: Envs/vec_env/vec_pretext_normalize.py:82-101 (getEmbeddings / calcReward), :47-59 (discounted-return
normalisation with clipping) and Envs/vec_env/running_mean_std.py:4-35 (streaming mean / variance).  The encoder
forward is the HIP path (VARPretextNet.forward); the rest is host arithmetic on (num_envs,) arrays in float64,
as in the reference.  IntrinsicReward(model, sound_sound=True) is config.RLRewardSoundSound: the current sound of every step
is embedded too and <current_sound_feat, goal_sound_feat> joins the reward, on the eager pair embeddings() / reward() and on the
captured step().  build_clip_table() embeds a pool of clips once per checkpoint (ClipTable); capture(batch, clip_table=table)
then takes clip indices instead of feature arrays (step_ids): no sound branch on the step, the goal cached per env.  Which C
entries a captured step is made of, route by route, is reward_step.py's business (RewardStep); this module owns the buffers.
"""
import numpy as np
import torch


class RunningMeanStd:
    """Streaming mean / variance of batches (parallel-variance update), running_mean_std.py:4-35."""

    def __init__(self, epsilon=1e-4, shape=()):
        self.mean = np.zeros(shape, np.float64)
        self.var = np.ones(shape, np.float64)
        self.count = epsilon

    def update(self, arr):
        arr = np.asarray(arr)
        self.update_from_moments(arr.mean(axis=0), arr.var(axis=0), arr.shape[0])

    def update_from_moments(self, batch_mean, batch_var, batch_count):
        delta = batch_mean - self.mean
        total = self.count + batch_count
        m2 = self.var * self.count + batch_var * batch_count + np.square(delta) * self.count * batch_count / total
        self.mean = self.mean + delta * batch_count / total
        self.var = m2 / total
        self.count = total


class ReturnNormalizer:
    """rew / sqrt(var(discounted return) + eps), clipped; returns reset where an episode ended
    (vec_pretext_normalize.py:47-59: gamma 0.99, cliprew 10, epsilon 1e-8)."""

    def __init__(self, num_envs, gamma=0.99, cliprew=10.0, epsilon=1e-8):
        self.ret_rms = RunningMeanStd(shape=())
        self.ret = np.zeros(num_envs)
        self.gamma, self.cliprew, self.epsilon = gamma, cliprew, epsilon

    def __call__(self, rews, news):
        rews = np.asarray(rews, dtype=np.float64)
        self.ret = self.ret * self.gamma + rews
        self.ret_rms.update(self.ret)
        out = np.clip(rews / np.sqrt(self.ret_rms.var + self.epsilon), -self.cliprew, self.cliprew)
        self.ret[np.asarray(news, dtype=bool)] = 0.0
        return out

    def reset(self):
        self.ret[:] = 0.0


def _arena_key(flat, params):
    """What a frozen model's arena is recognised by, besides the flat tensor itself: torch's version counters of it and of the
    parameters (load_state_dict, in-place ops; edits through .data bump nothing -- build the table again after those)."""
    return flat.data_ptr(), flat._version, sum([p._version for p in params])


class ClipTable:
    """The embeddings of a pool of sound clips under one frozen checkpoint (IntrinsicReward.build_clip_table): the env's
    sounds come from a finite, unaugmented pool (Envs/audioLoader.py:166-237) and the encoder does not change, so a clip's
    embedding is a constant and a reward step only needs the clip's index.

    feat: (rows + 1, dim) f32 on the device; row i is clip i, row `silent` (== rows) the embedding of the all-zero feature
    matrix the envs send when nothing is heard.  The table remembers the arena it was built from: used with a model whose
    arena has moved or changed since, it raises VarHipError -- build the table again (the pack-once rule's discipline)."""

    def __init__(self, feat, model):
        self.feat = feat
        self.rows = int(feat.shape[0]) - 1
        self.silent = self.rows
        self.dim = int(feat.shape[1])
        self._model = model
        self._flat = model.flat_parameters()
        self._params = list(model.parameters())                  # (the Parameter objects outlive load_state_dict and .to())
        self._key = _arena_key(self._flat, self._params)

    def check(self, model, flat=None):
        """Raises unless `model` still has the arena the table was built from; flat: model.flat_parameters() where the caller
        has just taken it (the walk over the modules is most of this check's cost on the step path)."""
        from ._lib import VarHipError
        flat = model.flat_parameters() if flat is None else flat
        if model is not self._model or flat is not self._flat or _arena_key(flat, self._params) != self._key:
            raise VarHipError("ClipTable: the encoder's parameter arena has moved or changed since the table was built "
                              "(load_state_dict, .to(), another model): build the table again")

    def host_ids(self, ids, name, batch, keep=False):
        """Host ids as a checked (batch,) int32 array; keep: -1 ("the cached goal of that env") is allowed.  A bad id raises."""
        from ._lib import VarHipError
        a = np.asarray(ids.numpy() if torch.is_tensor(ids) else ids)
        if a.shape != (batch,) or a.dtype.kind not in "iu":
            raise VarHipError(f"{name}: {batch} integer clip ids expected, got shape {a.shape} of {a.dtype}")
        lo = -1 if keep else 0
        if a.size and (a.min() < lo or a.max() > self.rows):
            raise VarHipError(f"{name}: ids outside {lo}..{self.rows} (rows 0..{self.rows - 1} are the clips, {self.rows} is "
                              f"silence{', -1 keeps the cached goal' if keep else ''}): {a.tolist()}")
        return a.astype(np.int32)

    def ids(self, ids, name, batch, keep=False):
        """One id argument of a step: an int32 device tensor as it is (a bad id there is the kernel's NaN rule), anything else
        range-checked on the host (host_ids) -- before anything is staged or copied."""
        return ids if torch.is_tensor(ids) and ids.is_cuda else self.host_ids(ids, name, batch, keep)


CLIP_CHUNK = 256        # clips embedded per call of build_clip_table: at most 25 MB (Kuka: 4) of features beside the table


class IntrinsicReward:
    """reward = env_reward + <image_feat, goal_sound_feat> (+ <current_sound_feat, goal_sound_feat> when
    sound_sound is on): getEmbeddings + calcReward of the reference wrapper, on the frozen HIP encoder.

    The goal sound of an episode is embedded once: pass goal_sound=None afterwards and the encoder returns the cached
    embedding (the reference signals this with an all-inf tensor, pretext_base.py:29-32; both are accepted)."""

    def __init__(self, model, representation_dim=3, sound_sound=False):
        self.model = model.eval()
        self.rep = representation_dim
        self.sound_sound = sound_sound

    @torch.no_grad()
    def embeddings(self, image_u8, goal_sound=None, current_sound=None):
        dev = next(self.model.parameters()).device
        to = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        img = to(image_u8)
        if img.dtype != torch.uint8:                  # the wrapper divides by 255 on the host; u8 goes in as is
            img = img.float().contiguous()
        goal = to(goal_sound)
        if goal is None:
            b = img.shape[0]
            goal = torch.full((b,) + tuple(self.model.config.sound_dim), float("inf"), device=dev)
        d = self.model(img, goal.float().contiguous(),
                       to(current_sound).float().contiguous() if (self.sound_sound and current_sound is not None) else None)
        image_feat = d["image_feat"].cpu().numpy()
        goal_feat = d["sound_feat_positive"].cpu().numpy()
        cur_feat = d["sound_feat_negative"].cpu().numpy() if (self.sound_sound and current_sound is not None) else 0.0
        return image_feat, goal_feat, cur_feat

    # ---- the clip table: every pool clip's embedding, once per checkpoint -------------------------------------
    @torch.no_grad()
    def build_clip_table(self, features=None, pcm=None, lens=None, chunk=CLIP_CHUNK):
        """Embed a pool of sound clips once -> ClipTable.  Either `features`, (rows,) + sound_dim precomputed feature matrices,
        or `pcm`, int16 (rows, stride) samples with `lens` (rows) -- a TripletPool's clips / clip_len as they are; PCM runs
        through ops.mfcc (Kuka: 100 frames) or ops.mfcc_psf (iTHOR: 600 frames) on the device.  Host arrays and device tensors
        are both taken; the work goes in chunks of `chunk` clips so that only a chunk's features exist at once.  The iTHOR
        encoder is var_ithor_reward_embed (the weights are packed here); the Kuka encoder var_arm_encoder_fwd with the clips as
        mfcc_pos alone, save_for_bwd = 2.  A row's bits do not depend on `chunk` or on its neighbours."""
        from ._lib import Context, VarHipError, current_stream_handle, ptr
        from .ithor import IthorVARPretextNet
        from .reward_step import prepare
        from . import ops
        m = self.model
        flat = m.flat_parameters()
        if not flat.is_cuda:
            raise VarHipError("IntrinsicReward.build_clip_table needs the model on the GPU (no CPU fallback)")
        if (features is None) == (pcm is None):
            raise VarHipError("IntrinsicReward.build_clip_table: features or pcm (with lens), one of the two")
        dev = flat.device
        sound_dim = tuple(m.config.sound_dim)
        src = features if pcm is None else pcm
        src = src if torch.is_tensor(src) else torch.from_numpy(np.ascontiguousarray(src))
        rows, chunk = int(src.shape[0]), int(chunk)
        if rows < 1 or chunk < 1:
            raise VarHipError("IntrinsicReward.build_clip_table: at least one clip and chunk >= 1")
        if pcm is None and (tuple(src.shape[1:]) != sound_dim or src.dtype != torch.float32):
            raise VarHipError(f"IntrinsicReward.build_clip_table: features are {src.dtype} {tuple(src.shape)}, expected float32 "
                              f"(rows,) + {sound_dim}")
        if pcm is not None:
            if src.dtype != torch.int16 or src.dim() != 2:
                raise VarHipError("IntrinsicReward.build_clip_table: pcm must be int16 (rows, stride)")
            if lens is None:
                lens = np.full(rows, src.shape[1], np.int32)
            lens = (lens if torch.is_tensor(lens) else torch.from_numpy(np.ascontiguousarray(lens))).to(torch.int32)
            if tuple(lens.shape) != (rows,):
                raise VarHipError(f"IntrinsicReward.build_clip_table: lens has shape {tuple(lens.shape)}, expected ({rows},)")
        ithor = isinstance(m, IthorVARPretextNet)
        c = Context.get(dev.index)
        w = prepare(c, m, flat, 16 if ithor else min(chunk, rows + 1))
        feat = torch.empty((rows + 1, self.rep), dtype=torch.float32, device=dev)

        def embed(x, out):
            n = x.shape[0]
            if ithor:
                c.check(c.lib.var_ithor_reward_embed(c.handle, current_stream_handle(), ptr(flat), ptr(x), n, ptr(out)),
                        "var_ithor_reward_embed")
                return
            w.bind()
            c.check(c.lib.var_arm_encoder_fwd(c.handle, current_stream_handle(), ptr(flat), None, 0, 0, ptr(x), None, n,
                                              int(m.config.img_dim[1]), None, ptr(out), None, None, None, 2), "var_arm_encoder_fwd")

        for at in range(0, rows, chunk):
            part = src[at:at + chunk].to(dev)
            if pcm is not None:
                front = ops.mfcc_psf if ithor else ops.mfcc
                part = front(part, lens[at:at + chunk].to(dev), out_frames=sound_dim[1])
            embed(part.contiguous(), feat[at:at + part.shape[0]])
        embed(torch.zeros((1,) + sound_dim, dtype=torch.float32, device=dev), feat[rows:])          # nothing is heard
        torch.cuda.current_stream().synchronize()                # (the chunks' features may be freed now)
        return ClipTable(feat, m)

    # ---- latency path: the whole frozen-encoder step as a replayed HIP graph --------------------------------
    def capture(self, batch, clip_table=None):
        """Capture the frozen encoder for a fixed number of envs (BASELINE config 5: 8) into two HIP graphs --
        image + goal sound (first step of an episode) and image only (later steps: the goal embedding is reused) --
        over static device buffers; the launches of each are reward_step.RewardStep's.  Weights are packed once here:
        call again after loading another checkpoint.  Returns self; then use step().

        For an IthorVARPretextNet (96 x 96 images, at most 64 envs) the arena is snapshotted, so the graphs follow the
        weights the model had at this call until capture() is called again.  The goal embedding is cached for the WHOLE
        batch (pretext_base.py:26-32: every env resets at the same time); step(image, None) before any goal step raises.

        With sound_sound (config.RLRewardSoundSound) both graphs also embed the current sound of every step and the reward
        is calcReward's <image_feat, goal_feat> + <current_sound_feat, goal_feat> (var_reward_dots' grouping).  Further
        static buffers, as attributes: current_sound (B,) + sound_dim, cur_feat (B,3), img_sound_dot and sound_sound_dot (B,).

        With clip_table (build_clip_table) the sounds arrive as clip indices: ONE graph, no sound branch in it, static int32
        buffers goal_ids / current_ids (B,), and step_ids() instead of step().  Without it everything is as above."""
        from ._lib import Context, VarHipError
        from .ithor import IthorVARPretextNet
        from .reward_step import RewardStep
        m, table, B, ss = self.model, clip_table, int(batch), bool(self.sound_sound)
        dev = m.flat_parameters().device
        if dev.type != "cuda":
            raise VarHipError("IntrinsicReward.capture needs the model on the GPU (no CPU fallback)")
        if table is not None and not isinstance(table, ClipTable):
            raise VarHipError("IntrinsicReward.capture: clip_table must be a ClipTable (build_clip_table)")
        if table is not None and (table.dim != 3 or table.feat.device != dev):
            raise VarHipError("IntrinsicReward.capture: the clip table is not this model's (dimension or device)")
        zeros = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)   # noqa: E731
        self._B, self._table, self._ithor = B, table, isinstance(m, IthorVARPretextNet)
        self._have_goal = False
        self._img = zeros(B, *m.config.img_dim, dtype=torch.uint8)
        self._image_feat, self._goal_feat, self._reward = zeros(B, 3), zeros(B, 3), zeros(B)
        self.current_sound = None                                # (set by a capture with sound_sound and no table)
        if table is None:
            self._goal = zeros(B, *m.config.sound_dim)
            goal, cur = self._goal, None
            if ss:
                cur = self.current_sound = zeros(B, *m.config.sound_dim)
        else:
            self._ids = torch.full((2, B), -1, dtype=torch.int32, device=dev)
            goal, cur = self.goal_ids, self.current_ids = self._ids[0], self._ids[1]
            cur.fill_(table.silent)
        if ss:
            self.cur_feat, self.img_sound_dot, self.sound_sound_dot = zeros(B, 3), zeros(B), zeros(B)
        c = Context.get(dev.index)
        more = dict(cur_feat=self.cur_feat, reward_img=self.img_sound_dot, reward_snd=self.sound_sound_dot) if ss else {}
        rs = self._step = RewardStep(c, m, B, image=self._img, is_u8=1, goal=goal, cur=cur, image_feat=self._image_feat,
                                     goal_feat=self._goal_feat, reward=self._reward, sound_sound=ss, clip_table=table, **more)
        keys = {"ids": True} if table is not None else {True: True, False: False}       # graph -> its with_goal
        with c.capturing() as graph:
            self._graphs = {key: graph(lambda g=with_goal: rs.launch(g, ss), warm=True) for key, with_goal in keys.items()}
            if self._ithor and table is None:
                self._goal_feat.zero_()                          # (the warm-up's embedding of the all-zero buffer is no goal)
        return self

    def _ids_input(self, ids, name, keep):
        """One id argument of step_ids (ClipTable.ids); an int32 tensor on the device must be this step's shape and device."""
        from ._lib import VarHipError
        ids = self._table.ids(ids, "IntrinsicReward.step_ids: " + name, self._B, keep)
        if torch.is_tensor(ids) and (ids.dtype != torch.int32 or tuple(ids.shape) != (self._B,) or ids.device != self._ids.device):
            raise VarHipError(f"IntrinsicReward.step_ids: {name} on the device must be int32 ({self._B},) on {self._ids.device}")
        return ids

    def step_ids(self, image_u8, goal_ids=None, current_ids=None):
        """One env step of a capture(batch, clip_table=table): clip indices instead of feature arrays.  goal_ids (B): a clip's
        row, table.silent, or -1 = keep the goal cached for THAT env; None = -1 everywhere.  current_ids (B): the sound heard
        in this step (table.silent when none); required with sound_sound, ignored without.  Host arrays are range-checked
        before anything is copied -- a bad id raises and changes nothing; int32 device tensors are taken as they are and a bad
        id there turns that env's outputs into NaN (include/var_hip.h).  A -1 for an env that never got a goal raises (ids on
        the device are not read back: after such a step every env counts as having one).  Returns (image_feat, goal_feat,
        reward) as step() does; cur_feat, img_sound_dot and sound_sound_dot are attributes when sound_sound is on."""
        from ._lib import VarHipError
        if "ids" not in getattr(self, "_graphs", {}):
            raise VarHipError("IntrinsicReward.step_ids: capture(batch, clip_table=table) first")
        self._table.check(self.model, self.model._flat)          # (.to() re-flattens at once: no walk over the modules per step)
        ss = bool(self.sound_sound)
        if ss and current_ids is None:
            raise VarHipError("IntrinsicReward.step_ids: sound_sound is on -- every step needs current_ids "
                              "(vec_pretext_normalize.py:82-95; table.silent when nothing is heard)")
        goal = np.full(self._B, -1, np.int32) if goal_ids is None else self._ids_input(goal_ids, "goal_ids", True)
        ids = [goal] + ([self._ids_input(current_ids, "current_ids", False)] if ss else [])
        kept = self._step.kept_goals(goal, "IntrinsicReward.step_ids", "pass their goal ids (pretext_base.py:26-32)")
        image_u8 = torch.as_tensor(image_u8)
        if tuple(image_u8.shape) != tuple(self._img.shape) or image_u8.dtype != torch.uint8:
            raise VarHipError(f"IntrinsicReward.step_ids: image is {image_u8.dtype} {tuple(image_u8.shape)}, expected uint8 "
                              f"{tuple(self._img.shape)}")
        if self._ithor and not image_u8.is_cuda:
            raise VarHipError("IntrinsicReward.step_ids: image must be a CUDA tensor (no CPU fallback)")
        self._img.copy_(image_u8, non_blocking=True)
        if not any(torch.is_tensor(a) for a in ids):             # all from the host: one copy for both
            self._ids[:len(ids)].copy_(torch.from_numpy(np.stack(ids)), non_blocking=True)
        else:
            for buf, a in zip(self._ids, ids):
                buf.copy_(a if torch.is_tensor(a) else torch.from_numpy(a), non_blocking=True)
        self._graphs["ids"].replay()
        self._step.goal_set |= ~kept
        return self._image_feat, self._goal_feat, self._reward

    def _checked(self, value, buf, name, strict):
        """One input of step() as a tensor; strict (iTHOR): a CUDA tensor of the buffer's shape, or a refusal."""
        from ._lib import VarHipError
        value = torch.as_tensor(value)
        if strict and not value.is_cuda:
            raise VarHipError(f"IntrinsicReward.step: {name} must be a CUDA tensor (no CPU fallback)")
        if (strict or buf is self.current_sound) and tuple(value.shape) != tuple(buf.shape):
            raise VarHipError(f"IntrinsicReward.step: {name} shape {tuple(value.shape)} is not {tuple(buf.shape)}")
        return value

    def step(self, image_u8, goal_sound=None, current_sound=None):
        """One env step of `batch` envs: copies the observations into the static buffers and replays the graph.
        Returns device tensors (image_feat (B,3), goal_feat (B,3), reward (B,)); they are overwritten by the next step.
        reward is <image_feat, goal_feat>; captured with sound_sound it is that plus <cur_feat, goal_feat> (the two terms
        stay in img_sound_dot / sound_sound_dot, the current sound's embedding in cur_feat) and every step needs
        current_sound -- without it the step raises before anything is copied or replayed.  Captured without sound_sound,
        current_sound is ignored, as embeddings() ignores it.  The iTHOR step takes CUDA tensors of the buffers' shapes only and
        refuses a step without any goal; the Kuka step copies what it is given, host arrays included."""
        from ._lib import VarHipError
        strict = self._ithor
        ss = self.current_sound is not None
        if ss and current_sound is None:
            raise VarHipError("IntrinsicReward.step: sound_sound is on -- every step needs current_sound "
                              "(vec_pretext_normalize.py:82-95)")
        copies = [(self._img, self._checked(image_u8, self._img, "image", strict))]
        if goal_sound is not None:
            copies.append((self._goal, self._checked(goal_sound, self._goal, "goal_sound", strict)))
        elif strict and not self._have_goal:
            raise VarHipError("IntrinsicReward.step: no goal embedding is cached yet -- pass goal_sound on the first "
                              "step of an episode (pretext_base.py:26-32)")
        if ss:
            copies.append((self.current_sound, self._checked(current_sound, self.current_sound, "current_sound", strict)))
        for buf, value in copies:
            buf.copy_(value, non_blocking=True)
        self._have_goal |= goal_sound is not None
        self._graphs[goal_sound is not None].replay()
        return self._image_feat, self._goal_feat, self._reward

    def reward(self, env_reward, image_feat, goal_feat, cur_feat=0.0):
        img_sound = np.sum(image_feat[:, :self.rep] * goal_feat, axis=1)
        snd_sound = np.sum(cur_feat * goal_feat, axis=1) if self.sound_sound else np.zeros_like(img_sound)
        return img_sound + snd_sound * float(self.sound_sound) + np.asarray(env_reward), img_sound, snd_sound

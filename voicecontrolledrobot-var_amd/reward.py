"""Frozen-encoder inference for the RL stage: embeddings, intrinsic reward and return-normalised reward
(BASELINE config 5).

Mirrors what the reference's vectorised-env wrapper does around the pretext model, without the simulator
plumbing: Envs/vec_env/vec_pretext_normalize.py:82-101 (getEmbeddings / calcReward), :47-59 (discounted-return
normalisation with clipping) and Envs/vec_env/running_mean_std.py:4-35 (streaming mean / variance).  The encoder
forward is the HIP path (VARPretextNet.forward); the rest is host arithmetic on (num_envs,) arrays in float64,
as in the reference.  IntrinsicReward(model, sound_sound=True) is config.RLRewardSoundSound: the current sound of every step
is embedded too and <current_sound_feat, goal_sound_feat> joins the reward, on the eager pair embeddings() / reward() and on the
captured step().
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

    # ---- latency path: the whole frozen-encoder step as a replayed HIP graph --------------------------------
    def capture(self, batch):
        """Capture the frozen encoder for a fixed number of envs (BASELINE config 5: 8) into two HIP graphs --
        image + goal sound (first step of an episode) and image only (later steps: the goal embedding is reused) --
        over static device buffers.  Weights are packed once here: call again after loading another checkpoint.
        Returns self; then use step().

        For an IthorVARPretextNet the step is var_ithor_reward_step (96 x 96 images, at most 64 envs): the arena is
        snapshotted and its convolutions packed once here, so the graphs follow the weights the model had at this call
        until capture() is called again.  The goal embedding is cached for the WHOLE batch (pretext_base.py:26-32:
        every env resets at the same time); step(image, None) before any goal step raises.

        With sound_sound (config.RLRewardSoundSound) both graphs also embed the current sound of every step and the reward
        is calcReward's <image_feat, goal_feat> + <current_sound_feat, goal_feat> (var_reward_dots' grouping).  Further
        static buffers, as attributes: current_sound (B,) + sound_dim, cur_feat (B,3), img_sound_dot and sound_sound_dot
        (B,).  The Kuka encoder takes the current sound as var_arm_encoder_fwd's mfcc_neg and var_reward_dots follows the
        forward (var_set_reward_dot is not armed); the iTHOR encoder is var_ithor_reward_step_ex."""
        from ._lib import Context, current_stream_handle, new_graph, ptr
        m = self.model
        from .ithor import IthorVARPretextNet
        self.current_sound = None                # (set by a capture with sound_sound)
        if isinstance(m, IthorVARPretextNet):
            return self._capture_ithor(batch)
        flat = m.flat_parameters()
        dev = flat.device
        c = Context.get(dev.index)
        hw = m.config.img_dim[1]
        B = int(batch)
        c.ensure_plan(B, hw)
        self._B = B
        self._img = torch.zeros((B, 3, hw, hw), dtype=torch.uint8, device=dev)
        self._goal = torch.zeros((B, 1, 100, 40), dtype=torch.float32, device=dev)
        self._image_feat = torch.zeros((B, 3), device=dev)
        self._goal_feat = torch.zeros((B, 3), device=dev)
        self._reward = torch.zeros((B,), device=dev)
        ss = bool(self.sound_sound)
        if ss:
            self._sound_sound_buffers(B, (1, 100, 40), dev)
        w = m.hip_weights(c, force=True)        # the frozen model's own packed image; the graphs keep its address

        def body(with_goal):
            w.bind()
            if ss:
                # the current sound rides as the forward's negative clip; both dots and their sum are one launch behind it
                c.check(c.lib.var_arm_encoder_fwd(c.handle, current_stream_handle(), ptr(flat), ptr(self._img), 1,
                                                  self._img.stride(0), ptr(self._goal) if with_goal else None,
                                                  ptr(self.current_sound), B, hw, ptr(self._image_feat),
                                                  ptr(self._goal_feat) if with_goal else None, ptr(self.cur_feat),
                                                  None, None, 2), "var_arm_encoder_fwd")
                c.check(c.lib.var_reward_dots(c.handle, current_stream_handle(), ptr(self._image_feat), ptr(self._goal_feat),
                                              ptr(self.cur_feat), B, self._image_feat.shape[1], ptr(self._reward),
                                              ptr(self.img_sound_dot), ptr(self.sound_sound_dot)), "var_reward_dots")
                return
            if not with_goal:
                # the goal embedding is cached: the forward itself leaves <image_feat, goal_feat> (var_set_reward_dot)
                c.check(c.lib.var_set_reward_dot(c.handle, ptr(self._goal_feat), ptr(self._reward)), "var_set_reward_dot")
            c.check(c.lib.var_arm_encoder_fwd(c.handle, current_stream_handle(), ptr(flat), ptr(self._img), 1,
                                              self._img.stride(0), ptr(self._goal) if with_goal else None, None, B, hw,
                                              ptr(self._image_feat), ptr(self._goal_feat) if with_goal else None,
                                              None, None, None, 2), "var_arm_encoder_fwd")      # 2: inference, small-batch kernels
            if not with_goal:
                return
            # <image_feat, goal_feat> (calcReward's torch.sum(a * b, dim=1): one launch instead of a product and a reduction)
            c.check(c.lib.var_row_dot(c.handle, current_stream_handle(), ptr(self._image_feat), ptr(self._goal_feat), B,
                                      self._image_feat.shape[1], ptr(self._reward)), "var_row_dot")

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        self._graphs = {}
        with torch.cuda.stream(side):
            for with_goal in (True, False):
                body(with_goal)                                  # warm-up outside capture (lazy kernel attributes)
                g = new_graph()
                with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                    body(with_goal)
                self._graphs[with_goal] = g
        torch.cuda.current_stream().wait_stream(side)
        return self

    def _capture_ithor(self, batch):
        from ._lib import Context, VarHipError, current_stream_handle, new_graph, ptr
        m = self.model
        flat = m.flat_parameters()
        dev = flat.device
        if not flat.is_cuda:
            raise VarHipError("IntrinsicReward.capture needs the model on the GPU (no CPU fallback)")
        c = Context.get(dev.index)
        if flat.numel() != c.lib.var_ithor_param_count():
            raise VarHipError("parameter arena does not match var_ithor_param_count()")
        hw = m.config.img_dim[1]
        B = int(batch)
        ss = bool(self.sound_sound)
        c.check(c.lib.var_ithor_reward_plan_ex(c.handle, B, int(hw), int(ss)), "var_ithor_reward_plan_ex")
        c.check(c.lib.var_ithor_reward_pack(c.handle, current_stream_handle(), ptr(flat)), "var_ithor_reward_pack")
        self._B = B
        self._ithor = True
        self._have_goal = False
        self._img = torch.zeros((B,) + tuple(m.config.img_dim), dtype=torch.uint8, device=dev)
        self._goal = torch.zeros((B,) + tuple(m.config.sound_dim), dtype=torch.float32, device=dev)
        self._image_feat = torch.zeros((B, 3), device=dev)
        self._goal_feat = torch.zeros((B, 3), device=dev)
        self._reward = torch.zeros((B,), device=dev)
        if ss:
            self._sound_sound_buffers(B, tuple(m.config.sound_dim), dev)

        def body(with_goal):
            if ss:
                c.check(c.lib.var_ithor_reward_step_ex(c.handle, current_stream_handle(), ptr(flat), ptr(self._img), 1,
                                                       self._img.stride(0), ptr(self._goal) if with_goal else None,
                                                       ptr(self.current_sound), B, ptr(self._image_feat), ptr(self._goal_feat),
                                                       ptr(self.cur_feat), ptr(self._reward), ptr(self.img_sound_dot),
                                                       ptr(self.sound_sound_dot)), "var_ithor_reward_step_ex")
                return
            c.check(c.lib.var_ithor_reward_step(c.handle, current_stream_handle(), ptr(flat), ptr(self._img), 1,
                                                self._img.stride(0), ptr(self._goal) if with_goal else None, B,
                                                ptr(self._image_feat), ptr(self._goal_feat), ptr(self._reward)),
                    "var_ithor_reward_step")

        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream())
        self._graphs = {}
        with torch.cuda.stream(side):
            for with_goal in (True, False):
                body(with_goal)                                  # warm-up outside capture (lazy kernel attributes)
                g = new_graph()
                with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                    body(with_goal)
                self._graphs[with_goal] = g
            self._goal_feat.zero_()                              # (the warm-up's embedding of the all-zero buffer is no goal)
        torch.cuda.current_stream().wait_stream(side)
        return self

    def _sound_sound_buffers(self, B, sound_dim, dev):
        self.current_sound = torch.zeros((B,) + tuple(sound_dim), dtype=torch.float32, device=dev)
        self.cur_feat = torch.zeros((B, 3), device=dev)
        self.img_sound_dot = torch.zeros((B,), device=dev)
        self.sound_sound_dot = torch.zeros((B,), device=dev)

    def _check_current(self, current_sound, cuda_only):
        """The current sound of a sound-sound step as a tensor, refused before anything is copied or replayed."""
        from ._lib import VarHipError
        if current_sound is None:
            raise VarHipError("IntrinsicReward.step: sound_sound is on -- every step needs current_sound "
                              "(vec_pretext_normalize.py:82-95)")
        current_sound = torch.as_tensor(current_sound)
        if cuda_only and not current_sound.is_cuda:
            raise VarHipError("IntrinsicReward.step: current_sound must be a CUDA tensor (no CPU fallback)")
        if tuple(current_sound.shape) != tuple(self.current_sound.shape):
            raise VarHipError(f"IntrinsicReward.step: current_sound shape {tuple(current_sound.shape)} is not "
                              f"{tuple(self.current_sound.shape)}")
        return current_sound

    def _step_ithor(self, image_u8, goal_sound, current_sound=None):
        from ._lib import VarHipError
        ss = getattr(self, "current_sound", None) is not None
        if ss:
            current_sound = self._check_current(current_sound, True)
        image_u8 = torch.as_tensor(image_u8)
        if not image_u8.is_cuda:
            raise VarHipError("IntrinsicReward.step: image must be a CUDA tensor (no CPU fallback)")
        if tuple(image_u8.shape) != tuple(self._img.shape):
            raise VarHipError(f"IntrinsicReward.step: image shape {tuple(image_u8.shape)} is not {tuple(self._img.shape)}")
        if goal_sound is not None:
            goal_sound = torch.as_tensor(goal_sound)
            if not goal_sound.is_cuda:
                raise VarHipError("IntrinsicReward.step: goal_sound must be a CUDA tensor (no CPU fallback)")
            if tuple(goal_sound.shape) != tuple(self._goal.shape):
                raise VarHipError(f"IntrinsicReward.step: goal_sound shape {tuple(goal_sound.shape)} is not "
                                  f"{tuple(self._goal.shape)}")
        elif not self._have_goal:
            raise VarHipError("IntrinsicReward.step: no goal embedding is cached yet -- pass goal_sound on the first "
                              "step of an episode (pretext_base.py:26-32)")
        self._img.copy_(image_u8, non_blocking=True)
        if goal_sound is not None:
            self._goal.copy_(goal_sound, non_blocking=True)
            self._have_goal = True
        if ss:
            self.current_sound.copy_(current_sound, non_blocking=True)
        self._graphs[goal_sound is not None].replay()
        return self._image_feat, self._goal_feat, self._reward

    def step(self, image_u8, goal_sound=None, current_sound=None):
        """One env step of `batch` envs: copies the observations into the static buffers and replays the graph.
        Returns device tensors (image_feat (B,3), goal_feat (B,3), reward (B,)); they are overwritten by the next step.
        reward is <image_feat, goal_feat>; captured with sound_sound it is that plus <cur_feat, goal_feat> (the two terms
        stay in img_sound_dot / sound_sound_dot, the current sound's embedding in cur_feat) and every step needs
        current_sound -- without it the step raises before anything is copied or replayed.  Captured without sound_sound,
        current_sound is ignored, as embeddings() ignores it."""
        if getattr(self, "_ithor", False):
            return self._step_ithor(image_u8, goal_sound, current_sound)
        if getattr(self, "current_sound", None) is not None:
            current_sound = self._check_current(current_sound, False)
            self.current_sound.copy_(current_sound, non_blocking=True)
        self._img.copy_(torch.as_tensor(image_u8), non_blocking=True)
        if goal_sound is not None:
            self._goal.copy_(torch.as_tensor(goal_sound), non_blocking=True)
        self._graphs[goal_sound is not None].replay()
        return self._image_feat, self._goal_feat, self._reward

    def reward(self, env_reward, image_feat, goal_feat, cur_feat=0.0):
        img_sound = np.sum(image_feat[:, :self.rep] * goal_feat, axis=1)
        snd_sound = np.sum(cur_feat * goal_feat, axis=1) if self.sound_sound else np.zeros_like(img_sound)
        return img_sound + snd_sound * float(self.sound_sound) + np.asarray(env_reward), img_sound, snd_sound

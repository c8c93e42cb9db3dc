"""The env wrapper's step on the device (csrc/env_step.hip; include/var_hip.h: var_reward_norm_step, var_rollout_move_at):
everything between "the simulator returned" and "the next act may run" -- the frozen encoder, calcReward, the return
normalisation, masks / bad_masks and RolloutStorage.insert (Envs/vec_env/vec_pretext_normalize.py:47-61, 96-101;
RL.py:137-141, 171-185) -- as ONE replayed HIP graph over buffers the act step and the storage already own.

    act = policy.capture(N, seed=0)                                  # ActStep
    rollouts = RolloutStorage(T, N, spaces, action_space, hidden, config, image_dtype=torch.uint8)
    collect = CollectStep(IntrinsicReward(encoder), act, rollouts)
    collect.reset(image, extras, goal_sound)                         # envs.reset() + RL.py:137-141
    for step in range(T):
        value, action, logp, hxs = act(act.obs, act.masks)           # replay 1
        image, extras, env_reward, done = simulator(action.cpu())    # the one host read of the step
        collect.observe(image, extras, env_reward, done)             # replay 2: nothing is read back

DeviceReturnNormalizer is the normaliser alone (reward.ReturnNormalizer with its state on the device).  GPU only: there is no
CPU fallback.  config.RLRewardSoundSound is IntrinsicReward(encoder, sound_sound=True): every observe() then takes the step's
current sound as well, the same replay embeds it and the normaliser's dot is <image_feat, goal_feat> +
<current_sound_feat, goal_feat>.  The encoder's launches, route by route, are reward_step.RewardStep's.  Not here: the act
replay inside the same graph (the value and action of slot T would be stale after the update) and _obfilt (off in both
reference configurations)."""
import numpy as np
import torch

from ._lib import Context, MoveAtSeg, MoveSeg, VarHipError, current_stream_handle, ptr
from .reward import ReturnNormalizer
from .reward_step import RewardStep

MAX_ENVS = 64                                                    # the reward step's limit (var_ithor_reward_plan; save_for_bwd = 2)
MAX_SEGS = 16                                                    # VAR_MOVE_MAX_SEGS
RMS_FRESH = (0.0, 1.0, 1e-4)                                     # RunningMeanStd(shape=()): mean, var, count


def _dev_tensor(t, name, device, dtypes, numel):
    if not torch.is_tensor(t) or not t.is_cuda or t.device != device:
        raise VarHipError(f"{name} must be a tensor on {device} (no CPU fallback)")
    if t.dtype not in dtypes or t.numel() != numel:
        raise VarHipError(f"{name} is {t.dtype} with {t.numel()} elements, expected {' / '.join(map(str, dtypes))} with {numel}")
    return t.detach().contiguous()


class DeviceReturnNormalizer:
    """reward.ReturnNormalizer (vec_pretext_normalize.py:47-59) with its state on the device: one launch of
    var_reward_norm_step per call, float64, the state bit for bit the host class's.

        norm = DeviceReturnNormalizer(num_envs)
        reward = norm(dot, env_reward, news)       # dot f32 (N) | None, env_reward f64 (N), news u8 / bool (N): device tensors
        reward = norm(rews, None, news)            # rews f64 (N): calcReward's sum already taken

    Returns the (N,1) float32 reward, a static buffer the next call overwrites; masks, bad_masks (N,1) f32 and orig_reward (N)
    f64 (origStepReward) are attributes.  episode (3,N) f64: the running sum of the un-normalised reward, the sum of the last
    finished episode and the number of finished episodes per env (RL.py:171-176)."""

    def __init__(self, num_envs, gamma=0.99, cliprew=10., epsilon=1e-8, device="cuda", num_steps=1, normalize=True):
        from .rollout import _device
        N = int(num_envs)
        if not 1 <= N <= 128 or int(num_steps) < 1:
            raise VarHipError("DeviceReturnNormalizer: 1 <= num_envs <= 128 (numpy's pairwise sum recurses beyond) and num_steps >= 1")
        dev = _device(device)
        self.device, self.num_envs, self.num_steps = dev, N, int(num_steps)
        self.gamma, self.cliprew, self.epsilon, self.normalize = float(gamma), float(cliprew), float(epsilon), bool(normalize)
        self._ctx = Context.get(dev.index)
        self._f64 = torch.zeros(5 * N + 3, dtype=torch.float64, device=dev)      # ret | rms | episode | orig_reward
        self.ret, self.rms = self._f64[:N], self._f64[N:N + 3]
        self.episode = self._f64[N + 3:4 * N + 3].view(3, N)
        self.orig_reward = self._f64[4 * N + 3:]
        self.rms.copy_(torch.tensor(RMS_FRESH, dtype=torch.float64))
        self.slot = torch.zeros(2, dtype=torch.int32, device=dev)
        self.reward, self.masks, self.bad_masks = (torch.zeros(N, 1, device=dev) for _ in range(3))

    def _launch(self, dot, env_reward, done, bad, masks=None):
        """The C call on prepared device tensors; masks: where the mask output goes (default self.masks)."""
        c = self._ctx
        c.check(c.lib.var_reward_norm_step(c.handle, current_stream_handle(), ptr(dot), ptr(env_reward), ptr(done), ptr(bad),
                                           self.num_envs, self.gamma, self.cliprew, self.epsilon, int(self.normalize), self.num_steps,
                                           ptr(self.ret), ptr(self.rms), ptr(self.episode), ptr(self.slot), ptr(self.reward),
                                           ptr(self.masks if masks is None else masks), ptr(self.bad_masks), ptr(self.orig_reward)),
                "var_reward_norm_step")

    def __call__(self, dot_or_rews, env_reward, news, bad=None):
        N, dev = self.num_envs, self.device
        if env_reward is None:
            dot, env_reward = None, _dev_tensor(dot_or_rews, "rews", dev, (torch.float64,), N)
        else:
            dot = None if dot_or_rews is None else _dev_tensor(dot_or_rews, "dot", dev, (torch.float32,), N)
            env_reward = _dev_tensor(env_reward, "env_reward", dev, (torch.float64,), N)
        u8 = lambda t, name: _dev_tensor(t, name, dev, (torch.uint8, torch.bool), N).view(torch.uint8)   # noqa: E731
        self._launch(dot, env_reward, u8(news, "news"), None if bad is None else u8(bad, "bad"))
        return self.reward

    def reset(self):
        self.ret.zero_()

    def state(self):
        """(mean, var, count, ret) as host float64 (blocking)."""
        h = self._f64[:self.num_envs + 3].cpu().numpy()
        N = self.num_envs
        return float(h[N]), float(h[N + 1]), float(h[N + 2]), h[:N].copy()

    def load(self, host):
        """Take over the state and constants of a reward.ReturnNormalizer; returns self."""
        if not isinstance(host, ReturnNormalizer) or np.shape(host.ret) != (self.num_envs,):
            raise VarHipError(f"DeviceReturnNormalizer.load: a ReturnNormalizer of {self.num_envs} envs")
        self.gamma, self.cliprew, self.epsilon = float(host.gamma), float(host.cliprew), float(host.epsilon)
        h = np.concatenate([np.asarray(host.ret, np.float64),
                            [float(host.ret_rms.mean), float(host.ret_rms.var), float(host.ret_rms.count)]])
        self._f64[:self.num_envs + 3].copy_(torch.from_numpy(h))
        return self

    def to_host(self):
        """A reward.ReturnNormalizer that continues this stream (blocking)."""
        mean, var, count, ret = self.state()
        host = ReturnNormalizer(self.num_envs, self.gamma, self.cliprew, self.epsilon)
        host.ret = ret
        host.ret_rms.mean, host.ret_rms.var, host.ret_rms.count = np.float64(mean), np.float64(var), count
        return host


def insert_segments(act, rollouts, reward, bad_masks):
    """The var_rollout_move_at table of RolloutStorage.insert (storage.py:61-77) fed from an act step's buffers:
    [(name, MoveAtSeg)] -- the observations, act's hidden state, masks and bad_masks go to slot + 1, action, log-prob, value and
    reward to slot; each destination is the store's slot 0, the stride one slot.  Works on any tensors with the act step's and
    the storage's attributes (the shapes are all it reads besides the addresses)."""
    N, T = rollouts.num_processes, rollouts.num_steps
    if not isinstance(rollouts.obs, dict):
        raise VarHipError("CollectStep: the storage must hold the observations as a dict (the policies' inputs)")
    missing = [k for k in rollouts.obs if k not in act.obs]
    if missing or len(rollouts.obs) != len(act.obs):
        raise VarHipError(f"CollectStep: the storage's observations {sorted(rollouts.obs)} are not the act step's {sorted(act.obs)}")
    rows = [(k, act.obs[k], rollouts.obs[k], 1) for k in rollouts.obs]
    rows += [("recurrent_hidden_states", act._hout, rollouts.recurrent_hidden_states, 1), ("actions", act.action, rollouts.actions, 0),
             ("action_log_probs", act.action_log_probs, rollouts.action_log_probs, 0), ("value_preds", act.value, rollouts.value_preds, 0),
             ("rewards", reward, rollouts.rewards, 0), ("masks", act.masks, rollouts.masks, 1),
             ("bad_masks", bad_masks, rollouts.bad_masks, 1)]
    if len(rows) > MAX_SEGS:
        raise VarHipError(f"CollectStep: {len(rows)} tensors per insert, one launch moves {MAX_SEGS}")
    table = []
    for name, src, store, add in rows:
        if src.dtype != store.dtype:
            what = "image dtype" if src.dim() >= 3 else "dtype"
            raise VarHipError(f"CollectStep: {name}: the storage's {what} {store.dtype} is not the act step's {src.dtype}")
        if store.shape[0] < T + add or store.shape[1] != N or src.numel() != store[0].numel() or src.shape[0] != N:
            raise VarHipError(f"CollectStep: {name}: the act step holds {tuple(src.shape)}, the storage {tuple(store.shape)}")
        if not src.is_contiguous() or not store.is_contiguous():
            raise VarHipError(f"CollectStep: {name} is not contiguous")
        rb = src.numel() // N * src.element_size()
        table.append((name, MoveAtSeg(MoveSeg(src.data_ptr(), store.data_ptr(), rb, 1, 0, 0, rb, rb), N * rb, add, T + add)))
    return table


class CollectStep:
    """One env step of the collection loop (RL.py:163-185 without the simulator) as one replay: the reward step of the frozen
    encoder (reward_step.RewardStep.launch: the entries of each route are listed there), var_reward_norm_step and one
    var_rollout_move_at, captured twice -- with and without a new goal sound.  The act step's own buffers are the operands:
    act_step.obs['image'] is the encoder's input, obs['image_feat'] / obs['goal_sound_feat'] its outputs (the cached goal
    embedding of the later steps lives there), act_step.masks the normaliser's mask output; nothing is copied between the parts.

    reward: an IntrinsicReward over a VARPretextNet or an IthorVARPretextNet with 96 x 96 images (its weights are packed
    here: build again after loading another checkpoint); act_step: policy.capture(N) of the matching policy; rollouts: a
    RolloutStorage whose image dtype is the act step's.  gamma, cliprew, epsilon, normalize: VecPretextNormalize's (normalize =
    its `ret`).  Refuses with VarHipError what it cannot run.

    reset(image, extras, goal_sound): envs.reset() + RL.py:137-141 (the reference discards the reset's reward, so it takes no
    current sound).  observe(image, extras, env_reward, done, bad=None, goal_sound=None, current_sound=None): one env step;
    with reward.sound_sound current_sound is required on every step -- self.dot then carries the sum of the two terms,
    self.dot_img / self.dot_snd the terms and self.cur_feat (N,3) the current sound's embedding -- and ignored otherwise.
    extras: {'robot_pose': (N,2)} (Kuka) / {'occupancy': (N,1,9,9)} (iTHOR).  Host arrays go through pinned staging buffers with non-blocking copies (an event guards the block's reuse); device tensors are copied, or
    used in place when they ARE the buffers (act_step.obs[...], self.env_reward, self.done, self.bad, self.goal_sound,
    self.current_sound).
    norm: the DeviceReturnNormalizer (reward, bad_masks, orig_reward, episode, state()); episode_stats() reads the episode block.

    clip_table (IntrinsicReward.build_clip_table of the same encoder): the sounds arrive as clip indices, not feature arrays --
    reset(image, extras, goal_ids=...), observe(..., goal_ids=None, current_ids=None); a goal id of -1 keeps THAT env's cached
    goal, so an env that starts an episode alone gets its new goal alone.  The replay holds no sound branch and is captured once
    -- the ids are read on the device -- beside the reset's; host ids ride in the small pinned block (2 * 4N bytes more, still
    one copy) and are range-checked before anything is staged; self.goal_ids / self.current_ids are the device buffers.
    Without clip_table everything is as described above."""

    def __init__(self, reward, act_step, rollouts, gamma=0.99, cliprew=10., epsilon=1e-8, normalize=True, clip_table=None):
        from .actor_critic import ActStep
        from .reward import ClipTable, IntrinsicReward
        from .rollout import RolloutStorage
        if not isinstance(reward, IntrinsicReward) or not isinstance(act_step, ActStep) or not isinstance(rollouts, RolloutStorage):
            raise VarHipError("CollectStep(reward: IntrinsicReward, act_step: ActStep, rollouts: RolloutStorage)")
        m = reward.model
        flat = m.flat_parameters()
        if not flat.is_cuda:
            raise VarHipError("CollectStep needs the encoder on the GPU: call .to('cuda') (no CPU fallback)")
        dev = flat.device
        N, T = act_step.batch, rollouts.num_steps
        if rollouts.device != dev or act_step.masks.device != dev:
            raise VarHipError("CollectStep: the encoder, the act step and the storage must live on one device")
        if tuple(m.config.img_dim[1:]) != tuple(act_step.obs['image'].shape[2:]):
            raise VarHipError(f"CollectStep: the encoder takes {tuple(m.config.img_dim[1:])} images, the policy "
                              f"{tuple(act_step.obs['image'].shape[2:])}")
        if N > MAX_ENVS:
            raise VarHipError(f"CollectStep: {N} envs, the reward step takes at most {MAX_ENVS}")
        if rollouts.num_processes != N:
            raise VarHipError(f"CollectStep: the storage holds {rollouts.num_processes} envs, the act step {N}")
        self.reward_model, self.act_step, self.rollouts = reward, act_step, rollouts
        self.device, self.num_envs = dev, N
        c = self._ctx = Context.get(dev.index)
        self.norm = DeviceReturnNormalizer(N, gamma, cliprew, epsilon, dev, num_steps=T, normalize=normalize)
        self._table = insert_segments(act_step, rollouts, self.norm.reward, self.norm.bad_masks)
        self._segs = (MoveAtSeg * len(self._table))(*(s for _, s in self._table))
        obs = act_step.obs
        self._extra = [k for k in obs if k not in ('image', 'image_feat', 'goal_sound_feat')]
        table = self.clip_table = clip_table
        if table is not None:
            if not isinstance(table, ClipTable) or table.dim != 3 or table.feat.device != dev:
                raise VarHipError("CollectStep: clip_table must be a ClipTable of this encoder (IntrinsicReward.build_clip_table)")
        else:
            self.goal_sound = torch.zeros((N,) + tuple(m.config.sound_dim), dtype=torch.float32, device=dev)
        self.dot = torch.zeros(N, device=dev)
        ss = self.sound_sound = bool(getattr(reward, "sound_sound", False))
        if ss:                                                   # RLRewardSoundSound: O['current_sound'] of every step, and what it adds
            if table is None:
                self.current_sound = torch.zeros_like(self.goal_sound)
            self.cur_feat = torch.zeros(N, 3, device=dev)
            self.dot_img, self.dot_snd = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
        # env_reward f64 | done u8 | bad u8: one device block, one staging copy; with a clip table the goal and the current ids
        # (i32 each) ride in it behind env_reward
        ids = 8 * N if table is not None else 0
        self._small = torch.zeros(8 * N + ids + 2 * N, dtype=torch.uint8, device=dev)
        self.env_reward = self._small[:8 * N].view(torch.float64)
        self.done, self.bad = self._small[8 * N + ids:9 * N + ids], self._small[9 * N + ids:]
        self._small_offs = {'env_reward': 0, 'done': 8 * N + ids, 'bad': 9 * N + ids}
        self._n_small = 3 if table is None else 4 + int(ss)      # what an observe() stages there: all from the host = one copy
        if table is not None:
            self.goal_ids = self._small[8 * N:12 * N].view(torch.int32)
            self.current_ids = self._small[12 * N:16 * N].view(torch.int32)
            self._small_offs.update(goal_ids=8 * N, current_ids=12 * N)
            self.goal_ids.fill_(-1)
            self.current_ids.fill_(table.silent)
            self._keep_ids = np.full(N, -1, np.int32)
        image, img_feat, goal_feat = obs['image'], obs['image_feat'], obs['goal_sound_feat']
        more = dict(cur_feat=self.cur_feat, reward_img=self.dot_img, reward_snd=self.dot_snd) if ss else {}
        goal, cur = (self.goal_sound, self.current_sound if ss else None) if table is None else (self.goal_ids, self.current_ids)
        rs = self._reward_step = RewardStep(c, m, N, image=image, is_u8=image.dtype == torch.uint8, goal=goal, cur=cur,
                                            image_feat=img_feat, goal_feat=goal_feat, reward=self.dot, sound_sound=ss,
                                            clip_table=table, **more)
        self._flat = rs.flat

        def body(with_goal):
            rs.launch(with_goal, True)
            self.norm._launch(self.dot, self.env_reward, self.done, self.bad, act_step.masks)
            c.check(c.lib.var_rollout_move_at(c.handle, current_stream_handle(), self._segs, len(self._segs),
                                              self.norm.slot.data_ptr() + 4, N), "var_rollout_move_at")

        bodies = {True: lambda: body(True), False: lambda: body(False), "reset": lambda: rs.launch(True, False)}
        if table is not None:                                    # the ids are read on the device: one body serves every kind of step
            bodies = {"step": lambda: body(True), "reset": lambda: rs.launch(True, False)}
        self._graphs = {}
        with c.capturing() as graph:
            keep = [(t, t.clone()) for t in (self.norm._f64, self.norm.slot, self.norm.reward, self.norm.bad_masks, act_step.masks,
                                             img_feat, goal_feat)]
            for key, fn in bodies.items():
                self.norm.slot.fill_(-2)                         # the warm-up's insert selects no slot: the storage stays as it is
                self._graphs[key] = graph(fn, warm=True)
            for t, saved in keep:                                # what the warm-up touched: ret, rms, episode, slot, the buffers
                t.copy_(saved)
            self.norm.slot.copy_(torch.tensor([rollouts.step, rollouts.step], dtype=torch.int32))
        self._slot = rollouts.step                               # host mirror of slot[0]
        self._have_goal = False
        # pinned staging: image | extras | goal sound | current sound (sound-sound) | env_reward, done, bad -- each 16-byte aligned
        self._stage, off = {}, 0
        sounds = [] if table is not None else [('goal_sound', self.goal_sound)] + ([('current_sound', self.current_sound)] if ss else [])
        for name, t in [('image', image)] + [(k, obs[k]) for k in self._extra] + sounds + [('small', self._small)]:
            self._stage[name] = (off, t)
            off += (t.numel() * t.element_size() + 15) // 16 * 16
        self._pin = torch.empty(off, dtype=torch.uint8).pin_memory()
        self._pin_np = self._pin.numpy()
        if table is not None:                                    # (the one copy moves the whole block: no stray ids from fresh memory)
            ids_np = self._pin_view('small')[1][8 * N:16 * N].view(np.int32)
            ids_np[:N], ids_np[N:] = -1, table.silent
        self._event = torch.cuda.Event()
        self._event_live = False

    # ---- staging ----------------------------------------------------------------------------------------------------------------
    def _pin_view(self, name):
        off, t = self._stage[name]
        n = t.numel() * t.element_size()
        return self._pin[off:off + n], self._pin_np[off:off + n]

    def _plan_input(self, name, value, buf):
        """Checks one input against its device buffer; returns None (it IS the buffer), ('dev', tensor) or ('host', array)."""
        if torch.is_tensor(value) and value.is_cuda:
            if value.device != self.device:
                raise VarHipError(f"CollectStep: {name} is on {value.device}, the step on {self.device}")
            if tuple(value.shape) != tuple(buf.shape) and value.numel() != buf.numel():
                raise VarHipError(f"CollectStep: {name} has shape {tuple(value.shape)}, the step takes {tuple(buf.shape)}")
            vd = torch.uint8 if value.dtype == torch.bool else value.dtype
            if vd != buf.dtype:
                raise VarHipError(f"CollectStep: {name} is {value.dtype}, the step takes {buf.dtype}")
            if value.data_ptr() == buf.data_ptr() and value.is_contiguous():
                return None
            return ('dev', value.detach().view(torch.uint8) if value.dtype == torch.bool else value.detach())
        if torch.is_tensor(value):
            value = value.detach().numpy()
        a = np.asarray(value)
        if a.size != buf.numel() or (a.ndim > 1 and tuple(a.shape) != tuple(buf.shape)):
            raise VarHipError(f"CollectStep: {name} has shape {a.shape}, the step takes {tuple(buf.shape)}")
        if (buf.dtype == torch.uint8) != (a.dtype in (np.uint8, np.bool_)):
            raise VarHipError(f"CollectStep: {name} is {a.dtype}, the step takes {buf.dtype}")
        return ('host', a)

    def _check_ready(self, slot=True):
        act = self.act_step
        if act.policy._flat is not act._flat or not act.policy._arena_intact():
            raise VarHipError("CollectStep: the policy's parameter arena has moved since capture(): capture and build again")
        if self.reward_model.model.flat_parameters() is not self._flat:
            raise VarHipError("CollectStep: the encoder's parameter arena has moved: build the CollectStep again")
        if slot and self.rollouts.step != self._slot:
            raise VarHipError(f"CollectStep: the storage is at step {self.rollouts.step}, the device slot at {self._slot}: "
                              "RolloutStorage.insert was called in between (reset() takes the storage's step over)")

    def _plans(self, image, extras, goal_sound, small, current_sound=None):
        obs = self.act_step.obs
        if not isinstance(extras, dict) or sorted(extras) != sorted(self._extra):
            raise VarHipError(f"CollectStep: extras must be a dict of {self._extra}")
        plans = [('image', self._plan_input('image', image, obs['image']), obs['image'])]
        plans += [(k, self._plan_input(k, extras[k], obs[k]), obs[k]) for k in self._extra]
        if goal_sound is not None:
            plans.append(('goal_sound', self._plan_input('goal_sound', goal_sound, self.goal_sound), self.goal_sound))
        if current_sound is not None:
            plans.append(('current_sound', self._plan_input('current_sound', current_sound, self.current_sound), self.current_sound))
        return plans + [(name, self._plan_input(name, v, buf), buf) for name, v, buf in small]

    def _stage_inputs(self, plans, small_names=()):
        """Host arrays -> the pinned block -> the device buffers (non-blocking), device tensors -> the buffers."""
        if self._event_live:
            self._event.synchronize()                            # the previous step's copies out of the block are done
        small = [(name, plan) for name, plan, _ in plans if name in small_names]
        packed = len(small) == self._n_small and all(plan is not None and plan[0] == 'host' for _, plan in small)
        offs = self._small_offs
        for name, plan, buf in plans:
            if plan is None or plan[0] != 'host':
                continue
            n = buf.numel() * buf.element_size()
            if name in small_names:
                pin, host = self._pin_view('small')
                pin, host = pin[offs[name]:offs[name] + n], host[offs[name]:offs[name] + n]
            else:
                pin, host = self._pin_view(name)
            np_dtype = {torch.uint8: np.uint8, torch.float32: np.float32, torch.float64: np.float64, torch.int32: np.int32}[buf.dtype]
            np.copyto(host.view(np_dtype), plan[1].reshape(-1), casting='unsafe')
            if not (packed and name in small_names):
                buf.view(-1).view(torch.uint8).copy_(pin, non_blocking=True)
        if packed:                                               # env_reward, done, bad: one copy when all three come from the host
            self._small.copy_(self._pin_view('small')[0], non_blocking=True)
        for name, plan, buf in plans:
            if plan is not None and plan[0] == 'dev':
                buf.view(-1).copy_(plan[1].reshape(-1), non_blocking=True)
        self._event.record()
        self._event_live = True

    # ---- the step ---------------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def reset(self, image, extras, goal_sound=None, goal_ids=None):
        """envs.reset() + RL.py:137-141: embeds the first observation (the goal sound with it), writes the observations to
        the storage's slot 0, zeroes the discounted return, sets act_step.masks to 1 (the storage's masks[0]) and takes the
        storage's step over as the device slot.  Built with a clip table it takes goal_ids (N), every env's goal clip, instead
        of goal_sound."""
        act, ro = self.act_step, self.rollouts
        self._check_ready(slot=False)
        if self.clip_table is not None:
            if goal_ids is None or goal_sound is not None:
                raise VarHipError("CollectStep.reset: built with a clip table -- the goal of every env comes as goal_ids")
            goal_ids = self.clip_table.ids(goal_ids, "CollectStep: goal_ids", self.num_envs)
            small = [('goal_ids', goal_ids, self.goal_ids)]
            plans = self._plans(image, extras, None, small)
            self._stage_inputs(plans, ('goal_ids',))
            self._reward_step.goal_set[:] = True
        else:
            if goal_sound is None:
                raise VarHipError("CollectStep.reset: the goal sound of the episode is required")
            plans = self._plans(image, extras, goal_sound, [])
            self._stage_inputs(plans)
        self._graphs["reset"].replay()
        ro._move([ro._slot_seg(act.obs[k], ro.obs[k][0]) for k in ro.obs], None, self.num_envs)
        self.norm.reset()
        act.masks.fill_(1.0)
        self.norm.slot.copy_(torch.tensor([ro.step, ro.step], dtype=torch.int32), non_blocking=False)
        self._slot = ro.step
        self._have_goal = True

    @torch.no_grad()
    def observe(self, image, extras, env_reward, done, bad=None, goal_sound=None, current_sound=None, goal_ids=None,
                current_ids=None):
        """One env step: obs, reward, done, infos of envs.step -> the storage (RL.py:164-185).  env_reward (N) float64, done /
        bad (N) uint8 or bool (bad: 'bad_transition' in info; None = none).  current_sound: O['current_sound'], required when the
        reward has sound_sound (a step without it raises and changes nothing: storage, normaliser and device slot stay) and
        ignored otherwise.  Returns the (N,1) float32 reward buffer; nothing is read back from the device.  The next act is
        act_step(act_step.obs, act_step.masks).

        Built with a clip table the sounds come as goal_ids / current_ids (N) instead: a goal id is a clip's row, table.silent,
        or -1 = that env keeps its cached goal (None: every env does), so an env that starts an episode alone gets its new goal
        alone; current_ids is required with sound_sound and ignored without.  Host ids are range-checked before anything is
        staged (a bad id raises and changes nothing) and ride in the one small copy; int32 device tensors are not read back."""
        self._check_ready()
        if self.clip_table is not None:
            return self._observe_ids(image, extras, env_reward, done, bad, goal_sound, current_sound, goal_ids, current_ids)
        if goal_ids is not None or current_ids is not None:
            raise VarHipError("CollectStep.observe: clip ids need a CollectStep built with clip_table")
        if self.sound_sound and current_sound is None:
            raise VarHipError("CollectStep.observe: the reward has sound_sound on -- every step needs current_sound "
                              "(vec_pretext_normalize.py:82-95)")
        if not self.sound_sound:
            current_sound = None
        if goal_sound is None and not self._have_goal:
            raise VarHipError("CollectStep.observe: no goal embedding is cached yet -- reset() or pass goal_sound "
                              "(pretext_base.py:26-32)")
        if bad is None:
            bad = self._zero_bad()
        small = [('env_reward', env_reward, self.env_reward), ('done', done, self.done), ('bad', bad, self.bad)]
        plans = self._plans(image, extras, goal_sound, small, current_sound)
        self._stage_inputs(plans, ('env_reward', 'done', 'bad'))
        self._graphs[goal_sound is not None].replay()
        self._have_goal = True
        self._slot = self.rollouts.step = (self._slot + 1) % self.rollouts.num_steps
        return self.norm.reward

    def _observe_ids(self, image, extras, env_reward, done, bad, goal_sound, current_sound, goal_ids, current_ids):
        self.clip_table.check(self.reward_model.model, self._flat)       # (_check_ready has just seen that the arena is self._flat)
        if goal_sound is not None or current_sound is not None:
            raise VarHipError("CollectStep.observe: built with a clip table -- the sounds come as goal_ids / current_ids")
        if self.sound_sound and current_ids is None:
            raise VarHipError("CollectStep.observe: the reward has sound_sound on -- every step needs current_ids "
                              "(vec_pretext_normalize.py:82-95; clip_table.silent when nothing is heard)")
        ids = lambda a, name, keep: self.clip_table.ids(a, "CollectStep: " + name, self.num_envs, keep)   # noqa: E731
        goal = self._keep_ids if goal_ids is None else ids(goal_ids, "goal_ids", True)
        kept = self._reward_step.kept_goals(goal, "CollectStep.observe", "reset() or pass their goal ids")
        if bad is None:
            bad = self._zero_bad()
        small = [('env_reward', env_reward, self.env_reward), ('goal_ids', goal, self.goal_ids)]
        if self.sound_sound:
            small.append(('current_ids', ids(current_ids, "current_ids", False), self.current_ids))
        small += [('done', done, self.done), ('bad', bad, self.bad)]
        plans = self._plans(image, extras, None, small)
        self._stage_inputs(plans, tuple(name for name, _, _ in small))
        self._graphs["step"].replay()
        self._reward_step.goal_set |= ~kept
        self._slot = self.rollouts.step = (self._slot + 1) % self.rollouts.num_steps
        return self.norm.reward

    def _zero_bad(self):
        z = getattr(self, "_bad0", None)
        if z is None:
            z = self._bad0 = np.zeros(self.num_envs, np.uint8)
        return z

    def episode_stats(self):
        """{'running', 'last', 'finished'}: (N,) float64 each -- the un-normalised reward of the running episode, of the last
        finished one, and the number of finished episodes per env (RL.py:171-176).  Blocking."""
        e = self.norm.episode.cpu().numpy()
        return {"running": e[0].copy(), "last": e[1].copy(), "finished": e[2].copy()}

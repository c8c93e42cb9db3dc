"""The PPO rollout around the networks, device-resident (csrc/rollout.hip; include/var_hip.h: var_rollout_move,
var_rollout_returns, var_ppo_head): drop-ins for the reference's models/ppo/storage.py:RolloutStorage and
models/ppo/algo/ppo.py:PPO, plus ppo_loss, the loss lines of ppo.py:66-87 as one launch with its gradients.

    rollouts = RolloutStorage(T, N, obs_shape, action_space, hidden, config, device="cuda", image_dtype=torch.uint8)
    step = policy.capture(N)                                        # ActStep: its static buffers go straight into insert
    value, action, logp, hxs = step(obs, masks)
    rollouts.insert(obs, hxs, action, logp, value, reward, masks, bad_masks)          # ONE launch
    rollouts.compute_returns(next_value, use_gae, gamma, gae_lambda)                  # ONE launch, advantages included
    agent = PPO(reference_policy, ...); agent.update(rollouts); rollouts.after_update()

The networks' evaluation forward and backward stay in PyTorch autograd: PPO takes the reference's Policy (the state_dict
of ArmNetPolicy / IthorNetPolicy loads into it unchanged) or any module with the same .base / .dist.  ppo_head_linear
(csrc/ppo_step.hip: var_ppo_head_linear) is ppo_loss with the distribution head's Linear in front of it, PPO(..., fused_head=True)
uses it, and PPO.capture(rollouts) replays whole minibatch steps as graphs (update_step.py).  GPU only: there is no
CPU fallback, CPU tensors raise VarHipError."""
import torch
import torch.nn as nn
import torch.optim as optim

from ._lib import Context, MoveSeg, VarHipError, current_stream_handle, ptr
from .optim import ClipAdam

MAX_SEGS = 16                                                    # VAR_MOVE_MAX_SEGS


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda" or not torch.cuda.is_available():
        raise VarHipError(f"the rollout lives on the GPU (device={device!r}): there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)


def _shape_of(space):
    return tuple(space.shape) if hasattr(space, "shape") else tuple(space)


class RolloutStorage:
    """models/ppo/storage.py:13-245 with the reference's attribute names, shapes and method signatures, resident on `device`
    from construction.  insert, after_update, compute_returns and each minibatch of recurrent_generator are one launch each.

    obs_shape: a dict of spaces / shapes (keys in config.RLObsIgnore are left out, as the reference) or anything else, which
    the reference turns into its flat (6 + 9*9 + 3*96*96,) layout.  image_dtype: the dtype of the observation members with
    three or more dimensions (torch.uint8 to store what ActStep is fed), or a dict {key: dtype}; the rest is float32.
    insert() takes device tensors of the stored dtype and size (ActStep's static buffers as they are); it copies, so the
    buffers may be overwritten by the next step.
    compute_returns() also leaves the normalised advantages of ppo.py:39-41, read with advantages().
    recurrent_generator() draws torch.randperm(num_processes) from the CPU generator where the reference does: a seeded run
    sees the same minibatches.  When num_mini_batch does not divide num_processes the reference's loop indexes past its
    permutation and raises on the last, short minibatch; here that minibatch is yielded with the envs that are left."""

    def __init__(self, num_steps, num_processes, obs_shape, action_space, recurrent_hidden_state_size, config,
                 device="cuda", image_dtype=torch.float32):
        T, N = int(num_steps), int(num_processes)
        if T < 1 or N < 1:
            raise VarHipError("RolloutStorage: num_steps and num_processes must be >= 1")
        dev = _device(device)
        self.device = dev
        self._ctx = Context.get(dev.index)
        z = lambda *shape, dtype=torch.float32: torch.zeros(shape, dtype=dtype, device=dev)      # noqa: E731
        if isinstance(obs_shape, dict):
            self.obs = {}
            for key in obs_shape:
                if key not in getattr(config, "RLObsIgnore", ()):
                    shape = _shape_of(obs_shape[key])
                    if isinstance(image_dtype, dict):
                        dt = image_dtype.get(key, torch.float32)
                    else:
                        dt = image_dtype if len(shape) >= 3 else torch.float32
                    self.obs[key] = z(T + 1, N, *shape, dtype=dt)
        else:
            self.obs = z(T + 1, N, int(6 + 9 * 9 + 3 * 96 * 96))
        self.recurrent_hidden_states = z(T + 1, N, int(recurrent_hidden_state_size))
        self.rewards = z(T, N, 1)
        self.value_preds = z(T + 1, N, 1)
        self.returns = z(T + 1, N, 1)
        self.action_log_probs = z(T, N, 1)
        if action_space.__class__.__name__ == 'Discrete':
            self.actions = z(T, N, 1, dtype=torch.int64)
        else:
            self.actions = z(T, N, int(action_space.shape[0]))
        self.masks = torch.ones(T + 1, N, 1, device=dev)
        self.bad_masks = torch.ones(T + 1, N, 1, device=dev)
        self._advantages = z(T, N, 1)
        self._have_advantages = False
        self.num_steps = T
        self.num_processes = N
        self.step = 0

    def to(self, device):
        if _device(device) != self.device:
            raise VarHipError("RolloutStorage lives on the device it was built on")

    # ---- one launch of var_rollout_move per 16 (src, dst) pairs ---------------------------------------------------------------
    def _obs_items(self, obs=None):
        if isinstance(self.obs, dict):
            if obs is not None:
                missing = [k for k in self.obs if k not in obs]
                if missing:
                    raise VarHipError(f"RolloutStorage: obs lacks {missing}")
            return [(k, self.obs[k], None if obs is None else obs[k]) for k in self.obs]
        return [("obs", self.obs, obs)]

    def _checked(self, t, like, name):
        """A device tensor holding one (N, ...) slot of `like`."""
        if not torch.is_tensor(t) or not t.is_cuda or t.device != self.device:
            raise VarHipError(f"RolloutStorage: {name} must be a tensor on {self.device} (no CPU fallback)")
        if t.dtype != like.dtype or t.numel() != like[0].numel():
            raise VarHipError(f"RolloutStorage: {name} is {t.dtype} {tuple(t.shape)}, the storage holds {like.dtype} "
                              f"{tuple(like.shape[1:])} per step")
        return t.detach().contiguous()

    def _move(self, segs, ind, n_env):
        c = self._ctx
        for i in range(0, len(segs), MAX_SEGS):
            part = segs[i:i + MAX_SEGS]
            table = (MoveSeg * len(part))(*part)
            c.check(c.lib.var_rollout_move(c.handle, current_stream_handle(), table, len(part), ind, n_env, self.num_processes),
                    "var_rollout_move")

    def _slot_seg(self, src, dst):
        """One (N, ...) slot -> one (N, ...) slot, env rows."""
        rb = dst.numel() // self.num_processes * dst.element_size()
        return MoveSeg(src.data_ptr(), dst.data_ptr(), rb, 1, 0, 0, rb, rb)

    def insert(self, obs, recurrent_hidden_states, actions, action_log_probs, value_preds, rewards, masks, bad_masks):
        s = self.step
        pairs = [(self._checked(o, store, k), store[s + 1]) for k, store, o in self._obs_items(obs)]
        for t, store, slot, name in ((recurrent_hidden_states, self.recurrent_hidden_states, s + 1, "recurrent_hidden_states"),
                                     (actions, self.actions, s, "actions"),
                                     (action_log_probs, self.action_log_probs, s, "action_log_probs"),
                                     (value_preds, self.value_preds, s, "value_preds"), (rewards, self.rewards, s, "rewards"),
                                     (masks, self.masks, s + 1, "masks"), (bad_masks, self.bad_masks, s + 1, "bad_masks")):
            pairs.append((self._checked(t, store, name), store[slot]))
        self._move([self._slot_seg(src, dst) for src, dst in pairs], None, self.num_processes)
        self.step = (s + 1) % self.num_steps

    def after_update(self):
        stores = [store for _, store, _ in self._obs_items()] + [self.recurrent_hidden_states, self.masks, self.bad_masks]
        self._move([self._slot_seg(x[-1], x[0]) for x in stores], None, self.num_processes)

    def compute_returns(self, next_value, use_gae, gamma, gae_lambda, use_proper_time_limits=True):
        """storage.py:89-128 (bit-equal to it) and the advantages of ppo.py:39-41, one launch."""
        c, T, N = self._ctx, self.num_steps, self.num_processes
        if not torch.is_tensor(next_value) or not next_value.is_cuda or next_value.device != self.device:
            raise VarHipError(f"RolloutStorage: next_value must be a tensor on {self.device} (no CPU fallback)")
        if next_value.dtype != torch.float32 or next_value.numel() != N:
            raise VarHipError(f"RolloutStorage: next_value is {next_value.dtype} {tuple(next_value.shape)}, expected float32 ({N}, 1)")
        nv = next_value.detach().contiguous()
        adv = self._advantages if T * N >= 2 else None           # (one value has no standard deviation: torch gives NaN)
        c.check(c.lib.var_rollout_returns(c.handle, current_stream_handle(), ptr(self.rewards), ptr(self.value_preds),
                                          ptr(self.masks), ptr(self.bad_masks), ptr(nv), T, N, int(bool(use_gae)), float(gamma),
                                          float(gae_lambda), int(bool(use_proper_time_limits)), ptr(self.returns), ptr(adv)),
                "var_rollout_returns")
        self._have_advantages = adv is not None

    def advantages(self):
        """(T, N, 1): (A - A.mean()) / (A.std() + 1e-5), A = returns[:-1] - value_preds[:-1], as of the last compute_returns."""
        if not self._have_advantages:
            raise VarHipError("RolloutStorage.advantages: call compute_returns first (num_steps * num_processes >= 2)")
        return self._advantages

    def feed_forward_generator(self, advantages, num_mini_batch=None, mini_batch_size=None):
        raise NotImplementedError("both policies (arm_VAR, ai2thor_VAR) are recurrent, so PPO.update never takes the "
                                  "feed-forward generator (models/ppo/algo/ppo.py:48-53): use recurrent_generator")

    def recurrent_generator(self, advantages, num_mini_batch):
        T, N, dev = self.num_steps, self.num_processes, self.device
        assert N >= num_mini_batch, (
            "PPO requires the number of processes ({}) to be greater than or equal to the number of "
            "PPO mini batches ({}).".format(N, num_mini_batch))
        if (not torch.is_tensor(advantages) or advantages.device != dev or advantages.dtype != torch.float32
                or advantages.numel() != T * N):
            raise VarHipError(f"recurrent_generator: advantages must be a float32 ({T}, {N}, 1) tensor on {dev}")
        advantages = advantages.detach().contiguous()
        num_envs_per_batch = N // num_mini_batch
        perm = torch.randperm(N)
        ind = perm.to(torch.int32).to(dev)
        full = [(k, store) for k, store, _ in self._obs_items()]
        full += [("actions", self.actions), ("value_preds", self.value_preds), ("returns", self.returns), ("masks", self.masks),
                 ("action_log_probs", self.action_log_probs), ("advantages", advantages)]
        for start_ind in range(0, N, num_envs_per_batch):
            nb = min(num_envs_per_batch, N - start_ind)
            out, segs = {}, []
            for k, store in full:
                rb = store[0, 0].numel() * store.element_size()
                o = out[k] = torch.empty((T * nb, *store.shape[2:]), dtype=store.dtype, device=dev)
                segs.append(MoveSeg(store.data_ptr(), o.data_ptr(), rb, T, N * rb, nb * rb, rb, rb))
            h = self.recurrent_hidden_states
            hb = h.shape[2] * h.element_size()
            hxs = torch.empty((nb, h.shape[2]), dtype=h.dtype, device=dev)
            segs.append(MoveSeg(h.data_ptr(), hxs.data_ptr(), hb, 1, 0, 0, hb, hb))
            self._move(segs, ind.data_ptr() + 4 * start_ind, nb)
            obs_batch = {k: out[k] for k in self.obs} if isinstance(self.obs, dict) else out["obs"]
            yield (obs_batch, hxs, out["actions"], out["value_preds"], out["returns"], out["masks"], out["action_log_probs"],
                   out["advantages"])


class _PPOLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, head, logstd, value, action, old_logp, adv, returns, value_preds, kind, clip, vcoef, ecoef, clipped):
        if not head.is_cuda:
            raise VarHipError("ppo_loss: inputs must be CUDA tensors (no CPU fallback)")
        dev = head.device
        if head.dim() != 2:
            raise VarHipError(f"ppo_loss: head must be (M, n), got {tuple(head.shape)}")
        M, n = head.shape
        want_action = torch.float32 if kind == 0 else torch.int64

        def prep(t, numel, name, dtype=torch.float32):
            if not torch.is_tensor(t) or t.device != dev or t.dtype != dtype or t.numel() != numel:
                raise VarHipError(f"ppo_loss: {name} must be a {dtype} tensor of {numel} elements on {dev}")
            return t.detach().contiguous()

        if kind not in (0, 1):
            raise VarHipError("ppo_loss: kind is 0 (DiagGaussian) or 1 (Categorical)")
        h = prep(head, M * n, "head")
        ls = prep(logstd, n, "logstd") if kind == 0 else None
        v, ol, ad, rt = prep(value, M, "value"), prep(old_logp, M, "old_logp"), prep(adv, M, "adv"), prep(returns, M, "returns")
        vp = prep(value_preds, M, "value_preds") if clipped else None
        a = prep(action, M * n if kind == 0 else M, "action", want_action)
        out = torch.empty(4, dtype=torch.float32, device=dev)
        g_head, g_value = torch.empty_like(h), torch.empty_like(v)
        g_logstd = torch.empty_like(ls) if kind == 0 else None
        c = Context.get(dev.index)
        c.check(c.lib.var_ppo_head(c.handle, current_stream_handle(), int(kind), ptr(h), ptr(ls), ptr(v), ptr(a), ptr(ol), ptr(ad),
                                   ptr(rt), ptr(vp), int(n), int(M), float(clip), float(vcoef), float(ecoef), int(bool(clipped)),
                                   ptr(out), ptr(g_head), ptr(g_value), ptr(g_logstd), None),
                "var_ppo_head")
        ctx.save_for_backward(g_head, g_value, g_logstd)
        ctx.shapes = (head.shape, value.shape, None if logstd is None else logstd.shape)
        total, vl, al, ent = out[3], out[0], out[1], out[2]
        ctx.mark_non_differentiable(vl, al, ent)
        return total, vl, al, ent

    @staticmethod
    def backward(ctx, g_total, *_):
        g_head, g_value, g_logstd = ctx.saved_tensors
        hs, vs, ls = ctx.shapes
        gl = (g_logstd * g_total).view(ls) if g_logstd is not None and ctx.needs_input_grad[1] else None
        return ((g_head * g_total).view(hs), gl, (g_value * g_total).view(vs)) + (None,) * 10


def ppo_loss(head, logstd, value, action, old_logp, adv, returns, value_preds, *, kind, clip_param, value_loss_coef,
             entropy_coef, use_clipped_value_loss=True):
    """The loss of models/ppo/algo/ppo.py:66-87 on one minibatch, forward and gradient in ONE launch (var_ppo_head).
    head (M,n): the action mean (kind 0, DiagGaussian, with logstd of n elements) or the logits (kind 1, Categorical,
    logstd None); value, old_logp, adv, returns, value_preds (M,1); action float32 (M,n) / int64 (M,1).
    Returns (total, value_loss, action_loss, dist_entropy), total = value_loss * value_loss_coef + action_loss -
    dist_entropy * entropy_coef; total.backward() hands head, value and logstd the gradients the launch left (autograd's own
    at the clip and max kinks, include/var_hip.h), scaled by the incoming gradient.  The other three are detached."""
    return _PPOLoss.apply(head, logstd, value, action, old_logp, adv, returns, value_preds, int(kind), float(clip_param),
                          float(value_loss_coef), float(entropy_coef), bool(use_clipped_value_loss))


class _PPOHeadLinear(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, weight, bias, logstd, value, action, old_logp, adv, returns, value_preds, kind, clip, vcoef, ecoef,
                clipped):
        if not torch.is_tensor(features) or not features.is_cuda:
            raise VarHipError("ppo_head_linear: inputs must be CUDA tensors (no CPU fallback)")
        dev = features.device
        if features.dim() != 2 or features.shape[1] != 128:
            raise VarHipError(f"ppo_head_linear: features must be (M, 128), got {tuple(features.shape)}")
        if kind not in (0, 1):
            raise VarHipError("ppo_head_linear: kind is 0 (DiagGaussian) or 1 (Categorical)")
        if not torch.is_tensor(weight) or weight.dim() != 2 or weight.shape[1] != 128:
            raise VarHipError("ppo_head_linear: weight must be (n, 128), nn.Linear's layout")
        M, n = features.shape[0], weight.shape[0]
        want_action = torch.float32 if kind == 0 else torch.int64

        def prep(t, numel, name, dtype=torch.float32):
            if not torch.is_tensor(t) or t.device != dev or t.dtype != dtype or t.numel() != numel:
                raise VarHipError(f"ppo_head_linear: {name} must be a {dtype} tensor of {numel} elements on {dev}")
            return t.detach().contiguous()

        f, w, b = prep(features, M * 128, "features"), prep(weight, n * 128, "weight"), prep(bias, n, "bias")
        ls = prep(logstd, n, "logstd") if kind == 0 else None
        v, ol, ad, rt = prep(value, M, "value"), prep(old_logp, M, "old_logp"), prep(adv, M, "adv"), prep(returns, M, "returns")
        vp = prep(value_preds, M, "value_preds") if clipped else None
        a = prep(action, M * n if kind == 0 else M, "action", want_action)
        c = Context.get(dev.index)
        ws_bytes = c.lib.var_ppo_head_linear_workspace_bytes(int(kind), int(n), int(M))
        if ws_bytes < 0:
            raise VarHipError(f"ppo_head_linear: kind {kind} takes n in 1..{4 if kind == 0 else 16} and M >= 1 (n {n}, M {M})")
        e = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)          # noqa: E731
        out, head, g_f, g_w, g_b, g_value = e(4), e(M, n), e(M, 128), e(n, 128), e(n), e(M)
        g_logstd = e(n) if kind == 0 else None
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        c.check(c.lib.var_ppo_head_linear(c.handle, current_stream_handle(), int(kind), ptr(f), ptr(w), ptr(b), ptr(ls), ptr(v), ptr(a),
                                          ptr(ol), ptr(ad), ptr(rt), ptr(vp), int(n), int(M), float(clip), float(vcoef), float(ecoef),
                                          int(bool(clipped)), ptr(head), ptr(out), ptr(g_f), ptr(g_w), ptr(g_b), ptr(g_value),
                                          ptr(g_logstd), ptr(ws), int(ws_bytes), None, 0, None, 0),
                "var_ppo_head_linear")
        ctx.save_for_backward(g_f, g_w, g_b, g_value, g_logstd)
        ctx.shapes = (features.shape, weight.shape, bias.shape, value.shape, None if logstd is None else logstd.shape)
        total, vl, al, ent = out[3], out[0], out[1], out[2]
        ctx.mark_non_differentiable(vl, al, ent)
        return total, vl, al, ent

    @staticmethod
    def backward(ctx, g_total, *_):
        g_f, g_w, g_b, g_value, g_logstd = ctx.saved_tensors
        fs, ws, bs, vs, ls = ctx.shapes
        gl = (g_logstd * g_total).view(ls) if g_logstd is not None and ctx.needs_input_grad[3] else None
        return ((g_f * g_total).view(fs), (g_w * g_total).view(ws), (g_b * g_total).view(bs), gl,
                (g_value * g_total).view(vs)) + (None,) * 10


def ppo_head_linear(features, weight, bias, logstd, value, action, old_logp, adv, returns, value_preds, *, kind, clip_param,
                    value_loss_coef, entropy_coef, use_clipped_value_loss=True):
    """ppo_loss with the distribution head's Linear in front of it (var_ppo_head_linear): features (M,128) are the actor
    features, weight (n,128) / bias (n) dist.fc_mean's (kind 0) or dist.linear's (kind 1) parameters; the rest as ppo_loss.
    Returns (total, value_loss, action_loss, dist_entropy); total.backward() hands features, weight, bias, logstd and value the
    gradients the call left, scaled by the incoming gradient.  The losses are var_ppo_head's on the same head, bit for bit."""
    return _PPOHeadLinear.apply(features, weight, bias, logstd, value, action, old_logp, adv, returns, value_preds, int(kind),
                                float(clip_param), float(value_loss_coef), float(entropy_coef), bool(use_clipped_value_loss))


class PPO:
    """models/ppo/algo/ppo.py:6-104 over the device-resident RolloutStorage and ppo_loss.  actor_critic: the reference's
    Policy, or any module with is_recurrent, .base(obs, hxs, masks, infer=False) -> (value, actor_features, hxs, extra) and
    .dist holding .linear (Categorical) or .fc_mean and .logstd._bias (DiagGaussian).  Its forward and backward run in
    PyTorch autograd; clip_grad_norm_ and optim.Adam as the reference, or -- fused_optimizer=True -- both inside
    var_amd.ClipAdam.step(): two launches (optim.py), the step count and the learning rate on the device, self.optimizer.param_groups
    as update_linear_schedule expects them, state_dict in optim.Adam's layout.  PPO(var_amd.bind_forward_gru(actor_critic), ...) puts
    the recurrent sequence of that evaluation (NNBase._forward_gru) on var_amd.masked_gru: forward and backward in HIP, no
    host read inside the update (gru_seq.py).  PPO(var_amd.bind_trunk(actor_critic), ...) puts the whole trunk behind imgCNN there,
    forward and backward (trunk.py), and trains an ArmNetPolicy / IthorNetPolicy in place.  fused_head=True: dist.fc_mean / dist.linear
    and its backward run inside the loss's call (ppo_head_linear), not as torch ops in front of ppo_loss."""

    def __init__(self, actor_critic, clip_param, ppo_epoch, num_mini_batch, value_loss_coef, entropy_coef, lr=None, eps=None,
                 max_grad_norm=None, use_clipped_value_loss=True, config=None, fused_optimizer=False, fused_head=False):
        self.config = config
        self.actor_critic = actor_critic
        self.clip_param = clip_param
        self.ppo_epoch = ppo_epoch
        self.num_mini_batch = num_mini_batch
        self.value_loss_coef = value_loss_coef
        self.entropy_coef = entropy_coef
        self.max_grad_norm = max_grad_norm
        self.use_clipped_value_loss = use_clipped_value_loss
        if not getattr(actor_critic, "is_recurrent", False):
            raise NotImplementedError("PPO: a recurrent actor-critic (both VAR policies are): the feed-forward generator is not provided")
        dist = actor_critic.dist
        if hasattr(dist, "fc_mean"):
            self._kind = 0
        elif hasattr(dist, "linear"):
            self._kind = 1
        else:
            raise NotImplementedError("PPO: actor_critic.dist must be the reference's DiagGaussian or Categorical")
        self.fused_optimizer = bool(fused_optimizer)
        self.fused_head = bool(fused_head)
        if self.fused_optimizer:
            self.optimizer = ClipAdam(actor_critic.parameters(), lr=lr, eps=eps, max_norm=max_grad_norm,
                                      policy=actor_critic if hasattr(actor_critic, "_arena_intact") else None)
        else:
            self.optimizer = optim.Adam(actor_critic.parameters(), lr=lr, eps=eps)

    def _head(self, feats):
        dist = self.actor_critic.dist
        if self._kind == 0:
            return dist.fc_mean(feats), dist.logstd._bias
        return dist.linear(feats), None

    def loss(self, sample):
        """(total, value_loss, action_loss, dist_entropy) of one minibatch of recurrent_generator."""
        obs, hxs, actions, value_preds, returns, masks, old_logp, adv = sample
        values, feats, _, _ = self.actor_critic.base(obs, hxs, masks, infer=False)
        if self.fused_head:
            dist = self.actor_critic.dist
            lin, logstd = (dist.fc_mean, dist.logstd._bias) if self._kind == 0 else (dist.linear, None)
            return ppo_head_linear(feats, lin.weight, lin.bias, logstd, values, actions, old_logp, adv, returns, value_preds,
                                   kind=self._kind, clip_param=self.clip_param, value_loss_coef=self.value_loss_coef,
                                   entropy_coef=self.entropy_coef, use_clipped_value_loss=self.use_clipped_value_loss)
        head, logstd = self._head(feats)
        return ppo_loss(head, logstd, values, actions, old_logp, adv, returns, value_preds, kind=self._kind,
                        clip_param=self.clip_param, value_loss_coef=self.value_loss_coef, entropy_coef=self.entropy_coef,
                        use_clipped_value_loss=self.use_clipped_value_loss)

    def capture(self, rollouts, precision=None):
        """The minibatch step of update(rollouts) as replayed graphs (update_step.py: UpdateStep), which update() then uses for
        this storage.  Needs a policy bound with bind_convs, fused_optimizer=True, fused_head=True and the device-resident
        RolloutStorage; precision defaults to bind_convs'.  Anything else raises VarHipError before a launch."""
        from .update_step import UpdateStep
        self._captured = UpdateStep(self, rollouts, precision)
        return self._captured

    def update(self, rollouts):
        captured = getattr(self, "_captured", None)
        if captured is not None and rollouts is captured.storage:
            return captured.update(rollouts)
        advantages = rollouts.advantages()
        stats = []
        for _ in range(self.ppo_epoch):
            for sample in rollouts.recurrent_generator(advantages, self.num_mini_batch):
                total, value_loss, action_loss, dist_entropy = self.loss(sample)
                self.optimizer.zero_grad()
                total.backward()
                if not self.fused_optimizer:                     # (ClipAdam.step clips inside)
                    nn.utils.clip_grad_norm_(self.actor_critic.parameters(), self.max_grad_norm)
                self.optimizer.step()
                stats.append(torch.stack((value_loss, action_loss, dist_entropy)))
        num_updates = self.ppo_epoch * self.num_mini_batch
        sums = torch.stack(stats).sum(0).tolist()                # (the one host read of an update)
        return sums[0] / num_updates, sums[1] / num_updates, sums[2] / num_updates

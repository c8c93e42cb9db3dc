"""Drop-in for the acting half of the reference's `Policy(base='arm_VAR')` (models/ppo/model.py:15-69 over
models/RL/arm_RL_model.py:armNet_VAR, Kuka configuration): same constructor arguments, module tree and state_dict
keys (63 tensors -- the authors' RL checkpoints load unchanged), `act` / `get_value` / `is_recurrent` /
`recurrent_hidden_state_size`.  The forward (8 convolutions, 3 max pools, the MLPs, one GRU step, value head, actor
trunk, DiagGaussian mean) is ONE C-ABI call, var_armnet_forward (csrc/armnet.hip); sampling and log-probabilities
(a handful of flops on (B,2) tensors) use torch.distributions exactly as the reference's FixedNormal does.
capture(num_envs) returns an ActStep: the same act() as ONE replayed HIP graph over static buffers -- the forward, then
var_policy_dist (csrc/policy_dist.hip: sampling from a seeded on-device generator or the mode, the log-probabilities and
the carry of the hidden state) -- for the RL loop's per-step latency; act() itself is unchanged.
Inference only: evaluate_actions raises -- the PPO update is var_amd.PPO (rollout.py) over the reference Policy, whose
evaluation forward and backward stay in PyTorch autograd -- or var_amd.PPO(var_amd.bind_trunk(policy), ...) over THIS object:
bind_trunk gives .base a differentiable forward (imgCNN in PyTorch, everything behind it in csrc/trunk.hip).  GPU only.

IthorNetPolicy is the same for base 'ai2thor_VAR' (models/RL/ai2thor_RL_model.py:ai2thorNet_VAR, iTHOR configuration,
Discrete actions: 64 tensors, var_ithor_policy_forward in csrc/ithor_policy.hip, sampling through
torch.distributions.Categorical as the reference's FixedCategorical).  Policy() dispatches on `base` as the reference's
Policy does.
set_acting_precision("bf16") (attribute acting_precision, default "fp32"; capture(..., precision=...) for one step) makes act,
get_value and capture round the operands of every imgCNN convolution to bf16 where bind_convs(policy, precision="bf16") rounds them
in the PPO update's evaluation (var_*_forward_ex flags bit 0): acting and evaluation then compute one function."""
import numpy as np
import torch
import torch.nn as nn

from ._lib import Context, VarHipError, current_stream_handle, ptr

# the acting forwards' precisions -> flags of var_*_forward_ex (bit 0: bf16 operands in every imgCNN convolution, the rounding
# points of conv_stack_eval's / bind_convs' precision="bf16")
PRECISIONS = {"fp32": 0, "bf16": 1}


def _flags(precision, who):
    if precision not in PRECISIONS:
        raise VarHipError(f"{who}: precision {precision!r} is neither 'fp32' nor 'bf16'")
    return PRECISIONS[precision]


def _ortho(m, gain):
    nn.init.orthogonal_(m.weight.data, gain=gain)
    nn.init.constant_(m.bias.data, 0)
    return m


class _TrunkBase(nn.Module):
    """What armNet_VAR and ai2thorNet_VAR construct alike, in the reference's order: NNBase's GRU first (then the subclass's
    convolutions), then _build_trunk's gain sqrt(2) orthogonal Linear layers."""

    def __init__(self, config, recurrent, rin, rh, action_hidden):
        super().__init__()
        self.config = config
        self._recurrent, self._recurrent_size, self._action_hidden_size = recurrent, rh, action_hidden
        self.gru = nn.GRU(rin, rh)
        for name, p in self.gru.named_parameters():
            if 'bias' in name:
                nn.init.constant_(p, 0)
            elif 'weight' in name:
                nn.init.orthogonal_(p)

    def _build_trunk(self, motor, im_hidden):
        """motor: the widths of motorMlp; im_hidden: imgMotorMlp's hidden width."""
        rin, rh, g = self.gru.input_size, self._recurrent_size, float(np.sqrt(2))
        mlp = lambda *w: nn.Sequential(*(m for i, o in zip(w, w[1:]) for m in (_ortho(nn.Linear(i, o), g), nn.ReLU())))  # noqa: E731
        self.motorMlp = mlp(*motor)
        self.cnnMlp = mlp(1152, 512, 256)
        self.imgMotorMlp = mlp(256, im_hidden, rin)
        self.imgMotorMlp2 = mlp(rh, 256)
        self.soundMlp = mlp(3, 128, 256, 256)
        self.fusionMlp = mlp(256, 512, 256)
        self.mlp_all = mlp(256, 256, 128)
        self.actor = mlp(128, 128, self._action_hidden_size)
        self.critic = mlp(128, 128, 128)
        self.critic_linear = _ortho(nn.Linear(128, 1), g)


class _Base(_TrunkBase):
    """Parameter container with armNet_VAR's attribute names, construction order and initialisers."""

    def __init__(self, config, recurrent, rin, rh, action_hidden):
        super().__init__(config, recurrent, rin, rh, action_hidden)
        self.imgCNN = nn.Sequential(
            nn.Conv2d(3, 32, 3, stride=1, padding=1), nn.ReLU(), nn.Conv2d(32, 32, 3, stride=1, padding=1), nn.ReLU(),
            nn.MaxPool2d(2, stride=2),
            nn.Conv2d(32, 64, 3, stride=1, padding=1), nn.ReLU(), nn.Conv2d(64, 64, 3, stride=1, padding=1), nn.ReLU(),
            nn.MaxPool2d(2, stride=2),
            nn.Conv2d(64, 128, 3, stride=1, padding=1), nn.ReLU(), nn.Conv2d(128, 128, 3, stride=1, padding=1), nn.ReLU(),
            nn.MaxPool2d(2, stride=2),
            nn.Conv2d(128, 256, 3, stride=2, padding=0), nn.ReLU(), nn.Conv2d(256, 128, 3, stride=1, padding=0), nn.ReLU(),
            nn.Flatten())
        torch.rand((1, *config.img_dim))                      # the reference's shape probe draws here
        self.imgCNN_outputShape = torch.Size((1, 1152))
        self._build_trunk((config.representationDim + config.robotStateDim, 256, 512, 256), 256)


class _AddBias(nn.Module):
    def __init__(self, n):
        super().__init__()
        self._bias = nn.Parameter(torch.zeros(n).unsqueeze(1))


class _DiagGaussian(nn.Module):
    def __init__(self, num_inputs, num_outputs):
        super().__init__()
        self.fc_mean = _ortho(nn.Linear(num_inputs, num_outputs), 1)
        self.logstd = _AddBias(num_outputs)


class _ArenaPolicy(nn.Module):
    """The parameters live in one flat float32 arena (the C ABI's `params`), re-flattened after .to() / .cuda()."""

    def _flatten_params(self):
        params = [p for _, p in self.named_parameters()]
        flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=params[0].device)
        o = 0
        for p in params:
            flat[o:o + p.numel()].copy_(p.data.reshape(-1).float())
            p.data = flat[o:o + p.numel()].view(p.shape)
            o += p.numel()
        self._flat = flat

    def _arena_intact(self):
        o = self._flat.data_ptr()
        for _, p in self.named_parameters():
            if p.data_ptr() != o or p.dtype != torch.float32:
                return False
            o += 4 * p.numel()
        return True

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._flatten_params()
        return r

    def forward(self, inputs, rnn_hxs, masks):
        raise NotImplementedError                             # as the reference (models/ppo/model.py:55-56)

    # Per class: _C, the prefix of its C entry points; _INPUTS, observation name -> (shape after the batch dimension, whether it
    # is an image that may stay uint8: divided by 255 on the device).  Per instance: _count_args, what var_*_param_count takes;
    # _n_head, the width of the distribution's Linear layer.
    def _finish_init(self, count_args, n_head):
        self._count_args, self._n_head = count_args, n_head
        self.acting_precision = "fp32"
        self._flat = None
        self._plan = 0
        self._flatten_params()

    def set_acting_precision(self, precision):
        """"fp32" (the default) or "bf16": what act, get_value and capture compute imgCNN with.  "bf16" rounds the operands of
        every imgCNN convolution where bind_convs(policy, precision="bf16") rounds them in the PPO update's evaluation
        (include/var_hip.h, var_*_forward_ex flags bit 0), so the rollout's log-probabilities and the update's first evaluation
        come from one function; everything behind the convolutions stays fp32.  Returns the policy."""
        _flags(precision, "set_acting_precision")
        self.acting_precision = precision
        return self

    def _call(self, c, name, *args):
        fn = f"{self._C}_{name}"
        c.check(getattr(c.lib, fn)(c.handle, *args), fn)

    @property
    def is_recurrent(self):
        return True

    @staticmethod
    def _prep(t, shape, image=False):
        if not t.is_cuda:
            raise VarHipError("inputs must be CUDA tensors (no CPU fallback)")
        if image:
            return (t if t.dtype == torch.uint8 else t.float()).reshape(shape).contiguous()
        t = t.float().contiguous()
        if tuple(t.shape) != tuple(shape):
            raise VarHipError(f"expected shape {shape}, got {tuple(t.shape)}")
        return t

    def _ensure_plan(self, c, B):
        if self._flat.numel() != getattr(c.lib, self._C + "_param_count")(*self._count_args):
            raise VarHipError(f"parameter arena does not match {self._C}_param_count()")
        if self._plan < B:
            self._call(c, "plan", int(B))
            self._plan = B

    def _base_forward(self, inputs, rnn_hxs, masks, head=True):
        """(value, actor_features, action mean / logits or None without `head`, rnn_hxs_out) of one forward."""
        if not self._arena_intact():
            self._flatten_params()
        flat = self._flat
        if not flat.is_cuda:
            raise VarHipError(f"{type(self).__name__} runs on the GPU only: call .to('cuda') (no CPU fallback)")
        c = Context.get(flat.device.index)
        B, H = inputs['image'].shape[0], self.recurrent_hidden_state_size
        obs = {k: self._prep(inputs[k], (B, *tail), image) for k, (tail, image) in self._INPUTS.items()}
        hxs, m = self._prep(rnn_hxs, (B, H)), self._prep(masks, (B, 1))
        self._ensure_plan(c, B)
        out = lambda n: torch.empty((B, n), dtype=torch.float32, device=flat.device)   # noqa: E731
        value, feats, head_out, hout = out(1), out(128), out(self._n_head) if head else None, out(H)
        self._launch_forward(c, obs, hxs, m, value, feats, head_out, hout, _flags(self.acting_precision, "acting_precision"))
        return value, feats, head_out, hout

    def capture(self, batch, deterministic=False, seed=0, image_dtype=torch.uint8, precision=None):
        """act() for a fixed number of envs as one replayed HIP graph with on-device sampling: see ActStep.  image_dtype:
        what the image inputs ('image', iTHOR's 'occupancy') will be fed as (uint8, or float32 already divided by 255).
        'image_feat' and 'goal_sound_feat' may be the device tensors IntrinsicReward.step returned: no host round trip.
        precision: "fp32" / "bf16" for this step, default the policy's acting_precision (set_acting_precision)."""
        return ActStep(self, batch, deterministic, seed, image_dtype, self.acting_precision if precision is None else precision)

    def chain_status(self):
        """Status of the small-batch (B <= 8) MLP chain launch, a persistent kernel that needs its 128 workgroups resident at
        once: 1 = the most recent forward timed out (its outputs are NaN), 0x40000001 = an earlier one did since the last
        clear_chain_status(), 0 = never.  Blocking.  (The reference's Policy.act, models/ppo/model.py:57-69, cannot fail;
        a caller that shares the GPU checks this after a NaN value or once per rollout.)"""
        import ctypes
        w = ctypes.c_uint(0)
        self._call(Context.get(self._flat.device.index), "status", ctypes.byref(w))
        return int(w.value)

    def clear_chain_status(self):
        self._call(Context.get(self._flat.device.index), "clear_status")

    @torch.no_grad()
    def get_value(self, inputs, rnn_hxs, masks):
        return self._base_forward(inputs, rnn_hxs, masks, head=False)[0]

    def evaluate_actions(self, inputs, rnn_hxs, masks, action):
        raise NotImplementedError("the networks' evaluation forward and backward stay in PyTorch: load this state_dict into "
                                  "the reference Policy and train it with var_amd.PPO over var_amd.RolloutStorage (storage, "
                                  "returns and the PPO loss head run on the device)")


class ActStep:
    """One replayed Policy.act step over static device buffers, returned by ArmNetPolicy.capture / IthorNetPolicy.capture:
    var_*_forward followed by var_policy_dist (sampling or mode, log-probabilities, and the copy that carries rnn_hxs_out
    into the next step's rnn_hxs) captured into ONE HIP graph.

        step = policy.capture(num_envs, seed=0)
        value, action, action_log_probs, rnn_hxs = step(obs, masks)      # models/ppo/model.py:57-69

    The returned tensors ARE the static buffers: the next step overwrites them (clone what a rollout keeps).  The hidden
    state lives here: reset() zeroes or sets it, and a zero in `masks` resets that row inside the forward, as hxs * masks
    does (models/ppo/model.py:118).  The noise comes from the kernel's own counter-based generator (include/var_hip.h),
    keyed by `seed`, whose step advances on the device with every replay: the same seed gives the same action sequence;
    the stream of numbers is not torch's, the distributions are the same.
    obs, masks: the static input buffers; a tensor passed to step() that IS its buffer (the caller filled step.obs[...] in
    place) is not copied.  head: the action mean (B,n) / the logits (B,n) of the last step; noise: the z (B,n) / u (B,) it
    used; rng_step: the generator step it drew from (-1 before the first sampling step; reads the device, blocking);
    precision: "fp32" / "bf16", what the captured forward computes imgCNN with (set_acting_precision; fixed at capture).

    Weights: the forwards re-pack their filters inside every call, so parameters updated IN PLACE (the PPO optimiser's
    step, load_state_dict) are what the next replay computes with.  The graph holds the arena's address: after .to() /
    .cuda() / anything else that moves the parameters, step() raises VarHipError -- call capture() again."""

    def __init__(self, policy, batch, deterministic, seed, image_dtype, precision="fp32"):
        flags = _flags(precision, "capture")
        self.precision = precision
        if not policy._arena_intact():
            policy._flatten_params()
        flat = policy._flat
        if not flat.is_cuda:
            raise VarHipError(f"{type(policy).__name__}.capture needs the model on the GPU: call .to('cuda') (no CPU fallback)")
        B, seed = int(batch), int(seed)
        if B < 1 or not 0 <= seed < 1 << 64:
            raise VarHipError("capture: batch must be >= 1 and seed in [0, 2^64)")
        if image_dtype not in (torch.uint8, torch.float32):
            raise VarHipError("capture: image_dtype is torch.uint8 (divided by 255 on the device) or torch.float32")
        dev = flat.device
        c = Context.get(dev.index)
        policy._ensure_plan(c, B)
        self.policy, self.batch, self.deterministic, self.seed = policy, B, bool(deterministic), seed
        self._flat = flat                                         # (held: its address cannot be handed out again)
        kind, n, hidden, logstd, shapes = policy._step_spec(B, image_dtype)
        self.obs = {k: torch.zeros(shape, dtype=dt, device=dev) for k, (shape, dt) in shapes.items()}
        f32 = lambda *shape: torch.zeros(shape, dtype=torch.float32, device=dev)   # noqa: E731
        self.masks, self._hxs, self._hout = f32(B, 1), f32(B, hidden), f32(B, hidden)
        self.value, self.actor_features, self.head = f32(B, 1), f32(B, 128), f32(B, n)
        self.action = f32(B, n) if kind == 0 else torch.zeros((B, 1), dtype=torch.int64, device=dev)
        self.action_log_probs = f32(B, 1)
        self.noise = f32(B, n) if kind == 0 else f32(B)
        self._rng = torch.zeros(4, dtype=torch.int32, device=dev)
        self._rng0 = torch.from_numpy(np.array([seed & 0xffffffff, seed >> 32, 0, 0], dtype=np.uint32).view(np.int32)).to(dev)

        def body():
            policy._launch_forward(c, self.obs, self._hxs, self.masks, self.value, self.actor_features, self.head, self._hout, flags)
            c.check(c.lib.var_policy_dist(c.handle, current_stream_handle(), kind, ptr(self.head), ptr(logstd), n, B,
                                          int(self.deterministic), None, ptr(self._rng), ptr(self.noise), ptr(self.action),
                                          ptr(self.action_log_probs), ptr(self._hout), ptr(self._hxs), hidden),
                    "var_policy_dist")

        with c.capturing() as graph:
            self._graph = graph(body, warm=True)
            self._rng.copy_(self._rng0)                          # (the warm-up drew from step 0 and carried its state)
            self._hxs.zero_()

    @property
    def rng_step(self):
        w = self._rng.cpu().numpy().view(np.uint32)
        return ((int(w[3]) << 32) | int(w[2])) - 1

    @torch.no_grad()
    def reset(self, rnn_hxs=None):
        """Zero the carried hidden state, or set it to rnn_hxs (B, recurrent_hidden_state_size)."""
        if rnn_hxs is None:
            self._hxs.zero_()
        else:
            self._hxs.copy_(self._checked(rnn_hxs, self._hxs, "rnn_hxs"), non_blocking=True)

    @staticmethod
    def _checked(t, buf, name):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise VarHipError(f"ActStep: {name} must be a CUDA tensor (no CPU fallback)")
        if tuple(t.shape) != tuple(buf.shape):
            raise VarHipError(f"ActStep: {name} has shape {tuple(t.shape)}, the captured step takes {tuple(buf.shape)}")
        if (buf.dtype == torch.uint8) != (t.dtype == torch.uint8):
            raise VarHipError(f"ActStep: {name} is {t.dtype}, the step was captured for {buf.dtype} (capture(image_dtype=...))")
        return t

    @torch.no_grad()
    def step(self, obs, masks):
        """Copy obs (the dict act() takes, CUDA tensors) and masks (B,1) into the static buffers and replay:
        (value, action, action_log_probs, rnn_hxs), each overwritten by the next step."""
        pol = self.policy
        if pol._flat is not self._flat or not pol._arena_intact():
            raise VarHipError("ActStep: the policy's parameter arena has moved since capture() (.to(), re-flattened "
                              "parameters): call capture() again")
        missing = [k for k in self.obs if k not in obs]
        if missing:
            raise VarHipError(f"ActStep: obs lacks {missing}")
        src = {k: self._checked(obs[k], buf, k) for k, buf in self.obs.items()}
        m = self._checked(masks, self.masks, "masks")
        for k, buf in self.obs.items():
            if src[k] is not buf:
                buf.copy_(src[k], non_blocking=True)
        if m is not self.masks:
            self.masks.copy_(m, non_blocking=True)
        self._graph.replay()
        return self.value, self.action, self.action_log_probs, self._hout

    __call__ = step


class ArmNetPolicy(_ArenaPolicy):
    _C = "var_armnet"
    _INPUTS = {'image': ((-1, 96, 96), True), 'image_feat': ((3,), False), 'robot_pose': ((2,), False),
               'goal_sound_feat': ((3,), False)}

    def __init__(self, obs_shape, action_space, config=None, base='arm_VAR', base_kwargs=None):
        super().__init__()
        kw = dict(recurrent=False, recurrentInputSize=128, recurrentSize=128, actionHiddenSize=128)
        kw.update(base_kwargs or {})
        if base != 'arm_VAR' or action_space.__class__.__name__ != "Box":
            raise NotImplementedError("HIP policy: base 'arm_VAR' with a Box action space")
        n_act = int(action_space.shape[0])
        if (tuple(config.img_dim) != (3, 96, 96) or config.representationDim != 3 or config.robotStateDim != 2
                or not kw['recurrent'] or kw['recurrentInputSize'] != 128 or kw['recurrentSize'] != 512
                or kw['actionHiddenSize'] != 128 or n_act != 2):
            raise VarHipError("HIP armNet_VAR supports the Kuka configuration: img_dim (3,96,96), representationDim 3, "
                              "robotStateDim 2, recurrent 128 -> 512, actionHiddenSize 128, 2 actions")
        self.base = _Base(config, True, 128, 512, 128)
        self.dist = _DiagGaussian(128, n_act)
        self._finish_init((), n_act)

    @property
    def recurrent_hidden_state_size(self):
        return 512

    def _launch_forward(self, c, obs, hxs, masks, value, feats, mean, hout, flags=0):
        """The C call on prepared tensors (contiguous, on the arena's device); flags: var_armnet_forward_ex's."""
        image, B = obs['image'], obs['image'].shape[0]
        c.check(c.lib.var_armnet_forward_ex(c.handle, current_stream_handle(), ptr(self._flat), ptr(image),
                                            int(image.dtype == torch.uint8), image.stride(0), ptr(obs['image_feat']),
                                            ptr(obs['robot_pose']), ptr(obs['goal_sound_feat']), ptr(hxs), ptr(masks), B,
                                            ptr(value), ptr(feats), ptr(mean), ptr(hout), int(flags)),
                "var_armnet_forward_ex")

    def _step_spec(self, B, image_dtype):
        f = torch.float32
        return 0, 2, 512, self.dist.logstd._bias, {'image': ((B, 3, 96, 96), image_dtype), 'image_feat': ((B, 3), f),
                                                   'robot_pose': ((B, 2), f), 'goal_sound_feat': ((B, 3), f)}

    def _normal(self, mean):
        std = self.dist.logstd._bias.t().view(1, -1).expand_as(mean).exp()
        return torch.distributions.Normal(mean, std)

    @torch.no_grad()
    def act(self, inputs, rnn_hxs, masks, deterministic=False):
        """models/ppo/model.py:57-69: (value, action, action_log_probs, rnn_hxs)."""
        value, _feats, mean, rnn_hxs = self._base_forward(inputs, rnn_hxs, masks)
        dist = self._normal(mean)
        action = mean if deterministic else dist.sample()
        return value, action, dist.log_prob(action).sum(-1, keepdim=True), rnn_hxs


class _IthorBase(_TrunkBase):
    """Parameter container with ai2thorNet_VAR's attribute names, construction order and initialisers
    (models/RL/ai2thor_RL_model.py:7-85): NNBase's GRU first, default-initialised convolutions and occupancy MLP, gain
    sqrt(2) orthogonal Linear layers.  No shape probe draws in this model."""

    def __init__(self, config, rin, rh, action_hidden):
        super().__init__(config, True, rin, rh, action_hidden)
        self.imgCNN = nn.Sequential(
            nn.Conv2d(3, 32, 3, stride=1, padding=1), nn.ReLU(), nn.Conv2d(32, 32, 3, stride=1, padding=1), nn.ReLU(),
            nn.MaxPool2d(2, stride=2),
            nn.Conv2d(32, 64, 3, stride=1, padding=1), nn.ReLU(), nn.MaxPool2d(2, stride=2),
            nn.Conv2d(64, 64, 3, stride=1, padding=1), nn.ReLU(), nn.MaxPool2d(2, stride=2),
            nn.Conv2d(64, 128, 3, stride=1, padding=1), nn.ReLU(), nn.MaxPool2d(2, stride=2),
            nn.Conv2d(128, 128, 3, stride=2, padding=1), nn.ReLU(),
            nn.Flatten())
        self.occupancyCNNMLP = nn.Sequential(
            nn.Conv2d(1, 64, 3, stride=2, padding=1), nn.ReLU(), nn.Conv2d(64, 32, 3, stride=2, padding=1), nn.ReLU(),
            nn.Flatten(), nn.Linear(32 * 9, 128), nn.ReLU(), nn.Linear(128, 256), nn.ReLU())
        self._build_trunk((3, 64, 256), 64)


class _Categorical(nn.Module):
    def __init__(self, num_inputs, num_outputs):
        super().__init__()
        self.linear = _ortho(nn.Linear(num_inputs, num_outputs), 0.01)


class IthorNetPolicy(_ArenaPolicy):
    """Acting half of the reference's `Policy(base='ai2thor_VAR')` with a Discrete action space (models/ppo/model.py:15-69
    over models/RL/ai2thor_RL_model.py:ai2thorNet_VAR, iTHOR configuration: recurrent 128 -> 1024, actionHiddenSize 128).
    inputs: 'image' (B,3,96,96) and 'occupancy' (B,1,9,9), each uint8 (divided by 255 on the device) or float already
    divided as processAI2Thor leaves them; 'image_feat' (B,3), 'goal_sound_feat' (B,3)."""

    MAX_ACTIONS = 16
    _C = "var_ithor_policy"
    _INPUTS = {'image': ((3, 96, 96), True), 'occupancy': ((1, 9, 9), True), 'image_feat': ((3,), False),
               'goal_sound_feat': ((3,), False)}

    def __init__(self, obs_shape, action_space, config=None, base='ai2thor_VAR', base_kwargs=None):
        super().__init__()
        kw = dict(recurrent=False, recurrentInputSize=128, recurrentSize=128, actionHiddenSize=128)
        kw.update(base_kwargs or {})
        if base != 'ai2thor_VAR' or action_space.__class__.__name__ != "Discrete":
            raise NotImplementedError("HIP policy: base 'ai2thor_VAR' with a Discrete action space")
        n_act = int(action_space.n)
        if (config is None or tuple(config.img_dim) != (3, 96, 96) or getattr(config, 'representationDim', 3) != 3
                or not kw['recurrent'] or kw['recurrentInputSize'] != 128 or kw['recurrentSize'] != 1024
                or kw['actionHiddenSize'] != 128 or not 1 <= n_act <= self.MAX_ACTIONS):
            raise VarHipError("HIP ai2thorNet_VAR supports the iTHOR configuration: img_dim (3,96,96), representationDim 3, "
                              f"recurrent 128 -> 1024, actionHiddenSize 128, 1..{self.MAX_ACTIONS} discrete actions")
        self.n_actions = n_act
        self.base = _IthorBase(config, 128, 1024, 128)
        self.dist = _Categorical(128, n_act)
        self._finish_init((n_act,), n_act)

    @property
    def recurrent_hidden_state_size(self):
        return 1024

    def _launch_forward(self, c, obs, hxs, masks, value, feats, logits, hout, flags=0):
        """The C call on prepared tensors (contiguous, on the arena's device); flags: var_ithor_policy_forward_ex's."""
        image, occ, B = obs['image'], obs['occupancy'], obs['image'].shape[0]
        c.check(c.lib.var_ithor_policy_forward_ex(c.handle, current_stream_handle(), ptr(self._flat), self.n_actions, ptr(image),
                                                  int(image.dtype == torch.uint8), image.stride(0), ptr(occ),
                                                  int(occ.dtype == torch.uint8), ptr(obs['image_feat']),
                                                  ptr(obs['goal_sound_feat']), ptr(hxs), ptr(masks), B,
                                                  ptr(value), ptr(feats), ptr(logits), ptr(hout), int(flags)),
                "var_ithor_policy_forward_ex")

    def _step_spec(self, B, image_dtype):
        f = torch.float32
        return 1, self.n_actions, 1024, None, {'image': ((B, 3, 96, 96), image_dtype), 'occupancy': ((B, 1, 9, 9), image_dtype),
                                               'image_feat': ((B, 3), f), 'goal_sound_feat': ((B, 3), f)}

    @torch.no_grad()
    def act(self, inputs, rnn_hxs, masks, deterministic=False):
        """models/ppo/model.py:57-69: (value, action (B,1) int64, action_log_probs (B,1), rnn_hxs)."""
        value, _feats, logits, rnn_hxs = self._base_forward(inputs, rnn_hxs, masks)
        dist = torch.distributions.Categorical(logits=logits)             # FixedCategorical (models/ppo/distributions.py)
        action = dist.probs.argmax(dim=-1, keepdim=True) if deterministic else dist.sample().unsqueeze(-1)
        logp = dist.log_prob(action.squeeze(-1)).view(action.size(0), -1).sum(-1).unsqueeze(-1)
        return value, action, logp, rnn_hxs


def Policy(obs_shape, action_space, config=None, base=None, base_kwargs=None):
    """The reference's Policy(...) dispatch on `base` (models/ppo/model.py:15-45) onto the HIP policies."""
    policies = {'arm_VAR': ArmNetPolicy, 'ai2thor_VAR': IthorNetPolicy}
    if base not in policies:
        raise NotImplementedError(f"HIP policy: base {base!r} (supported: {sorted(policies)})")
    return policies[base](obs_shape, action_space, config=config, base=base, base_kwargs=base_kwargs)

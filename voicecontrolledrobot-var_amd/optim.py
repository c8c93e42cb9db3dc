"""The PPO update's optimiser step on the device (csrc/clip_adam.hip; include/var_hip.h: var_clip_adam_step): what
models/ppo/algo/ppo.py:89-91 does with nn.utils.clip_grad_norm_ and optim.Adam in a few dozen launches per minibatch, as two.

    opt = ClipAdam(policy.parameters(), lr=6e-5, eps=1e-5, max_norm=0.5)
    opt.zero_grad(); loss.backward(); total_norm = opt.step()              # total_norm: a device scalar, the unclipped norm

The step count and the learning rate live on the device, nothing is allocated by the library or read back, and equal inputs give
equal bits, so step() can sit inside a torch.cuda.graph capture.  The gradients are left as they are (PyTorch scales them in
place; nothing reads them afterwards).  GPU only, fp32 only: there is no CPU fallback, anything else raises VarHipError before a
launch.  (The table of step() is pointer arithmetic, so the table and state_dict can be
looked at on CPU tensors too; step() itself refuses them.)"""
import torch

from ._lib import Context, OptSeg, VarHipError, current_stream_handle, ptr

MAX_TABLE = 256                                                  # var_clip_adam_step takes up to 256 segments
_MOVED = ("ClipAdam: the policy's parameter arena has moved since the optimiser was built (.to(), re-flattened parameters): build "
          "the optimiser again")


class ClipAdam:
    """clip_grad_norm_(params, max_norm) (norm type 2; max_norm None: no clip) + torch.optim.Adam(params, lr, betas, eps).step()
    (weight decay 0, no amsgrad, no maximize) in one call of var_clip_adam_step.

    params: float32 parameters on one device (CUDA for step()).  exp_avg and exp_avg_sq are one flat tensor each, laid out in
    parameter order: an arena policy's parameters and moments are contiguous runs, and step() merges such neighbours into one
    segment.  param_groups is a list with one dict holding params, lr, betas and eps, so that the reference's
    update_linear_schedule (models/ppo/utils.py:45-49) works on it; a changed lr reaches the device by a launch at the next
    step(), never by a synchronising copy.  One step count serves all parameters: parameters whose .grad is None are left out as
    PyTorch leaves them out, and a step() whose set of parameters with gradients differs from the first step's raises
    VarHipError instead of silently diverging from PyTorch's per-parameter counts.  state_dict / load_state_dict use
    torch.optim.Adam's layout, so a run can move between the two optimisers in either direction.
    policy: an ArmNetPolicy / IthorNetPolicy whose parameters these are; step() then raises, as ActStep does, when its
    parameter arena has moved."""

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, max_norm=None, policy=None):
        params = list(params)
        if not params:
            raise VarHipError("ClipAdam: no parameters")
        for p in params:
            if not torch.is_tensor(p) or p.dtype != torch.float32 or p.device != params[0].device or p.is_sparse:
                raise VarHipError("ClipAdam: parameters must be dense float32 tensors on one device")
        if len({id(p) for p in params}) != len(params):
            raise VarHipError("ClipAdam: a parameter appears twice")
        if lr is None or eps is None or not lr >= 0 or not eps >= 0 or not all(0 <= b < 1 for b in betas):
            raise VarHipError(f"ClipAdam: lr {lr} (>= 0), betas {tuple(betas)} (in [0, 1)), eps {eps} (>= 0)")
        if max_norm is not None and not float(max_norm) > 0:
            raise VarHipError(f"ClipAdam: max_norm {max_norm} (> 0, or None for no clip)")
        dev = params[0].device
        self.max_norm = None if max_norm is None else float(max_norm)
        self.param_groups = [{"params": params, "lr": float(lr), "betas": (float(betas[0]), float(betas[1])), "eps": float(eps)}]
        total = sum(p.numel() for p in params)
        self.exp_avg = torch.zeros(total, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(total, dtype=torch.float32, device=dev)
        self._offsets, o = [], 0
        for p in params:
            self._offsets.append(o)
            o += p.numel()
        self._lr_dev = torch.full((1,), float(lr), dtype=torch.float32, device=dev)
        self._lr_written = float(lr)
        self._step_dev = torch.zeros(1, dtype=torch.int32, device=dev)
        self._norm = torch.zeros(1, dtype=torch.float32, device=dev)
        self._active = None                                      # indices of the parameters the first step() found gradients on
        self._held = None                                        # the last step's gradient tensors (a captured graph reads them)
        self._policy = policy
        self._numels = [p.numel() for p in params]
        # (the policy's own parameters, in its order: _table's walk over them then is the policy's _arena_intact())
        self._policy_walk = policy is not None and [id(p) for p in policy.parameters()] == [id(p) for p in params]

    # ---- the segment table ------------------------------------------------------------------------------------------------------
    def _moments(self, i):
        p, o = self.param_groups[0]["params"][i], self._offsets[i]
        return self.exp_avg[o:o + p.numel()], self.exp_avg_sq[o:o + p.numel()]

    def _table(self):
        """[(p_ptr, g_ptr, m_ptr, v_ptr, n)] of this step from the .grad tensors as they are -- neighbours whose four arrays all
        continue each other in memory merged into one segment -- and the gradient tensors it points into.  (On addresses: this
        loop is the host's share of a step, a microsecond or two per parameter.)  With a policy whose parameters these are, in order, the walk also is its _arena_intact()."""
        params = self.param_groups[0]["params"]
        f32, strided, dev = torch.float32, torch.strided, self.exp_avg.device
        m0, v0 = self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr()
        walk = self._policy is not None and self._policy_walk
        arena = self._policy._flat.data_ptr() if walk else 0
        active, segs, grads = [], [], []
        for i, p in enumerate(params):
            n, pp = self._numels[i], p.data_ptr()
            if walk:
                if pp != arena or p.dtype is not f32:
                    raise VarHipError(_MOVED)
                arena += 4 * n
            g = p.grad
            if g is None or n == 0:
                continue
            if g.dtype is not f32 or g.layout is not strided or g.device != dev or g.numel() != n:
                raise VarHipError(f"ClipAdam: the gradient of parameter {i} must be a dense float32 tensor of its size on {dev}")
            if not p.is_contiguous():
                raise VarHipError(f"ClipAdam: parameter {i} is not contiguous")
            if not g.is_contiguous():
                g = g.contiguous()
            active.append(i)
            grads.append(g)
            o = 4 * self._offsets[i]
            row = [pp, g.data_ptr(), m0 + o, v0 + o, n]
            if segs:
                last = segs[-1]
                k = 4 * last[4]
                if last[0] + k == row[0] and last[1] + k == row[1] and last[2] + k == row[2] and last[3] + k == row[3]:
                    last[4] += n
                    continue
            segs.append(row)
        if self._active is None:
            if not active:
                raise VarHipError("ClipAdam.step: no parameter has a gradient")
            self._active = tuple(active)
        elif tuple(active) != self._active:
            raise VarHipError("ClipAdam.step: the set of parameters that have gradients differs from the first step's (one step count "
                              "serves all parameters; torch.optim.Adam would count per parameter)")
        if len(segs) > MAX_TABLE:
            raise VarHipError(f"ClipAdam.step: {len(segs)} segments after merging, var_clip_adam_step takes {MAX_TABLE}")
        return [tuple(r) for r in segs], grads

    # ---- torch.optim.Optimizer's surface ---------------------------------------------------------------------------------------
    def zero_grad(self, set_to_none=True):
        for p in self.param_groups[0]["params"]:
            p.grad = None

    @torch.no_grad()
    def step(self):
        """One clip + Adam step; returns total_norm (a device scalar, overwritten by the next step), or None without max_norm."""
        group = self.param_groups[0]
        dev = self.exp_avg.device
        if dev.type != "cuda":
            raise VarHipError(f"ClipAdam.step runs on the GPU only (parameters on {dev}): there is no CPU fallback")
        pol = self._policy
        if pol is not None and not self._policy_walk and not pol._arena_intact():
            raise VarHipError(_MOVED)
        segs, grads = self._table()
        lr = float(group["lr"])
        if lr != self._lr_written:
            self._lr_dev.fill_(lr)                               # (a launch, stream-ordered in front of the step)
            self._lr_written = lr
        b1, b2 = group["betas"]
        c = Context.get(dev.index)
        table = (OptSeg * len(segs))(*(OptSeg(*s) for s in segs))
        c.check(c.lib.var_clip_adam_step(c.handle, current_stream_handle(), table, len(segs),
                                         0.0 if self.max_norm is None else self.max_norm, ptr(self._lr_dev), float(b1), float(b2),
                                         float(group["eps"]), ptr(self._step_dev), ptr(self._norm)),
                "var_clip_adam_step")
        self._held = grads
        return None if self.max_norm is None else self._norm[0]

    def step_count(self):
        """The number of steps taken (reads the device, blocking)."""
        return int(self._step_dev.item())

    def state_dict(self):
        """torch.optim.Adam's layout: state[i] = {step, exp_avg, exp_avg_sq} for the parameters that have been stepped, and
        param_groups with Adam's own keys (reads the step count from the device, blocking)."""
        group = self.param_groups[0]
        n = len(group["params"])
        like = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=group["lr"], betas=group["betas"], eps=group["eps"])
        pg = dict(like.state_dict()["param_groups"][0])
        pg["params"] = list(range(n))
        state, step = {}, self.step_count()
        if step > 0:
            for i in self._active or ():
                m, v = self._moments(i)
                shape = group["params"][i].shape
                state[i] = {"step": torch.tensor(float(step)), "exp_avg": m.clone().view(shape), "exp_avg_sq": v.clone().view(shape)}
        return {"state": state, "param_groups": [pg]}

    def load_state_dict(self, state_dict):
        groups = state_dict["param_groups"]
        params = self.param_groups[0]["params"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(params):
            raise VarHipError("ClipAdam.load_state_dict: one parameter group over the same number of parameters")
        g = groups[0]
        if g.get("weight_decay", 0) or g.get("amsgrad", False) or g.get("maximize", False):
            raise VarHipError("ClipAdam.load_state_dict: weight decay, amsgrad and maximize are not provided")
        index = {key: i for i, key in enumerate(g["params"])}
        state = {index[k]: s for k, s in state_dict["state"].items()}
        steps = {int(float(s["step"])) for s in state.values()}
        if len(steps) > 1:
            raise VarHipError(f"ClipAdam.load_state_dict: per-parameter step counts {sorted(steps)}: one step count serves all parameters")
        step = steps.pop() if steps else 0
        with torch.no_grad():
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
            for i, s in state.items():
                m, v = self._moments(i)
                m.copy_(s["exp_avg"].reshape(-1))
                v.copy_(s["exp_avg_sq"].reshape(-1))
            self._step_dev.fill_(step)
        self._active = tuple(sorted(state)) if step > 0 else None
        self.param_groups[0].update(lr=float(g["lr"]), betas=(float(g["betas"][0]), float(g["betas"][1])), eps=float(g["eps"]))

"""A whole PPO minibatch step as one replayed graph (PPO.capture -> UpdateStep): the gather of the minibatch
(var_rollout_move_cursor), the convolution stacks and the trunk forward, the head's Linear with the loss and its gradients
(var_ppo_head_linear), the trunk and the stacks backward, and the agent's own ClipAdam.step() -- the C entries called directly on
buffers that are allocated once, with no autograd graph, no allocation and no host read inside.

    agent = PPO(bind_convs(policy), ..., fused_optimizer=True, fused_head=True)
    step = agent.capture(rollouts)            # one graph per distinct minibatch env count (the short last minibatch has its own)
    agent.update(rollouts)                    # one upload of the permutations, ppo_epoch * minibatches replays, one host read

Which minibatch a replay works on is decided on the device: all epochs' permutations lie behind one index list, a cursor word
selects the env list of the gather, and the launch that writes the losses moves the cursor on and files the three statistics in
their row.  The step shares the agent's optimiser state (moments, step count, learning rate), so eager and captured steps may
alternate on one agent; it computes what the eager update with the same settings computes, bit for bit."""
import ctypes

import torch

from ._lib import Context, MoveSeg, VarHipError, current_stream_handle, ptr
from .convstack import PRECISIONS, _convs_forward, _flags, stack_parameters
from .rollout import MAX_SEGS, RolloutStorage
from .trunk import _LAYOUT, trunk_kind, trunk_parameters

_GAP = 64                                                        # floats between the gradient blocks: ClipAdam merges inside a block,
#                                                                  never across two, which is the eager path's table exactly


def _table(tensors):
    return (ctypes.c_void_p * len(tensors))(*(t.data_ptr() for t in tensors))


class _Minibatch:
    """The static buffers and the launch sequence of minibatches of `nb` envs."""

    def __init__(self, owner, nb):
        self.owner, self.nb = owner, nb
        ro, agent, dev, c = owner.storage, owner.agent, owner.device, owner._ctx
        base, dist = agent.actor_critic.base, agent.actor_critic.dist
        kind, T, N = owner.kind, ro.num_steps, ro.num_processes
        M = self.M = T * nb
        H = _LAYOUT[kind][0]
        lib = c.lib
        self.buffers = []

        def new(*shape, dtype=torch.float32):
            t = torch.zeros(shape, dtype=dtype, device=dev)
            self.buffers.append(t)
            return t

        def sized(n, what):
            if n < 0:
                raise VarHipError(f"PPO.capture: {what} refuses T {T}, {nb} envs per minibatch")
            return int(n)

        # the gathered minibatch (recurrent_generator's tensors)
        stores = [(k, store) for k, store, _ in ro._obs_items()]
        stores += [("actions", ro.actions), ("value_preds", ro.value_preds), ("returns", ro.returns), ("masks", ro.masks),
                   ("action_log_probs", ro.action_log_probs), ("advantages", ro._advantages)]
        if len(stores) + 1 > MAX_SEGS:
            raise VarHipError(f"PPO.capture: {len(stores) + 1} tensors per minibatch, one gather takes {MAX_SEGS}")
        self.mb, segs = {}, []
        for k, store in stores:
            rb = store[0, 0].numel() * store.element_size()
            o = self.mb[k] = new(M, *store.shape[2:], dtype=store.dtype)
            segs.append(MoveSeg(store.data_ptr(), o.data_ptr(), rb, T, N * rb, nb * rb, rb, rb))
        h = ro.recurrent_hidden_states
        hb = h.shape[2] * h.element_size()
        self.hxs = new(nb, h.shape[2])
        segs.append(MoveSeg(h.data_ptr(), self.hxs.data_ptr(), hb, 1, 0, 0, hb, hb))
        self._segs = (MoveSeg * len(segs))(*segs)
        self._held = [store for _, store in stores] + [h]        # (the graph reads them in place)
        if h.shape[2] != H:
            raise VarHipError(f"PPO.capture: the storage holds hidden states of {h.shape[2]}, the policy's are {H}")

        # the networks: convolution stacks, trunk
        obs = {k: self.mb[k] for k, _, _ in ro._obs_items()} if isinstance(ro.obs, dict) else None
        need = ["image", "image_feat", "goal_sound_feat"] + (["occupancy"] if kind else ["robot_pose"])
        if obs is None or any(k not in obs for k in need):
            raise VarHipError(f"PPO.capture: the storage's observations must hold {need}")
        for k in need:
            want = (torch.uint8, torch.float32) if k in ("image", "occupancy") else (torch.float32,)
            if obs[k].dtype not in want:
                raise VarHipError(f"PPO.capture: observation {k!r} is stored as {obs[k].dtype}")
        self.obs = obs
        self.stacks = []                                         # (kind, parameters, image, feat, saved, d_feat, gradient block)
        flags = owner.flags
        ws_bytes = 0
        for sk, module, key, width in ([(2, base.occupancyCNNMLP, "occupancy", 288)] if kind else []) + [(kind, base.imgCNN, "image", 1152)]:
            ps = stack_parameters(module, sk)
            offs = [lib.var_convstack_grad_offset(sk, i) for i in range(len(ps) + 1)]
            self.stacks.append(dict(kind=sk, params=ps, image=obs[key], feat=new(M, width), d_feat=new(M, width), offs=offs,
                                    saved=new(sized(lib.var_convstack_saved_floats(sk, M), "var_convstack_saved_floats"))))
            ws_bytes = max(ws_bytes, sized(lib.var_convstack_workspace_bytes_ex(sk, M, flags), "var_convstack_workspace_bytes_ex"))
        self.tp = trunk_parameters(base, kind)
        self.t_offs = [lib.var_trunk_grad_offset(kind, i) for i in range(len(self.tp) + 1)]
        self.motor_in = new(M, 5) if kind == 0 else obs["image_feat"]
        self.value, self.feats, self.h_T, self.d_hxs = new(M, 1), new(M, 128), new(nb, H), new(nb, H)
        self.t_saved = new(sized(lib.var_trunk_saved_floats(kind, T, nb), "var_trunk_saved_floats"))
        ws_bytes = max(ws_bytes, sized(lib.var_trunk_workspace_bytes(kind, T, nb), "var_trunk_workspace_bytes"))
        # the head
        lin = dist.fc_mean if agent._kind == 0 else dist.linear
        self.lin, self.logstd = lin, dist.logstd._bias if agent._kind == 0 else None
        n = self.n = lin.weight.shape[0]
        if tuple(lin.weight.shape) != (n, 128):
            raise VarHipError(f"PPO.capture: the head's Linear is {tuple(lin.weight.shape)}, (n, 128) expected")
        self.head, self.out, self.g_features, self.g_value = new(M, n), new(4), new(M, 128), new(M)
        ws_bytes = max(ws_bytes, sized(lib.var_ppo_head_linear_workspace_bytes(agent._kind, n, M), "var_ppo_head_linear_workspace_bytes"))
        self.ws = new(ws_bytes, dtype=torch.uint8)               # (the launches follow each other on one stream: one workspace)
        # one flat gradient buffer, a block per entry in the order of the sequence's parameters, p.grad as views of it
        blocks = [("stack", s) for s in self.stacks] + [("trunk", None), ("W", None), ("b", None)] + ([("logstd", None)] if agent._kind == 0 else [])
        sizes = [b[1]["offs"][-1] if b[0] == "stack" else {"trunk": self.t_offs[-1], "W": n * 128, "b": n, "logstd": n}[b[0]] for b in blocks]
        starts, o = [], 0
        for sz in sizes:
            starts.append(o)
            o += (sz + _GAP + 63) // 64 * 64
        self.grad_flat = new(o)
        self.grads = {}                                          # id(parameter) -> its view of grad_flat
        for (what, s), at in zip(blocks, starts):
            if what == "stack":
                s["g"] = self.grad_flat[at:at + s["offs"][-1]]
                for i, p in enumerate(s["params"]):
                    self.grads[id(p)] = s["g"][s["offs"][i]:s["offs"][i] + p.numel()].view(p.shape)
            elif what == "trunk":
                self.t_g = self.grad_flat[at:at + self.t_offs[-1]]
                for i, p in enumerate(self.tp):
                    self.grads[id(p)] = self.t_g[self.t_offs[i]:self.t_offs[i] + p.numel()].view(p.shape)
            else:
                p = {"W": lin.weight, "b": lin.bias, "logstd": self.logstd}[what]
                g = self.grad_flat[at:at + p.numel()]
                setattr(self, "g_" + what, g)
                self.grads[id(p)] = g.view(p.shape)
        params = list(agent.actor_critic.parameters())
        missing = [i for i, p in enumerate(params) if id(p) not in self.grads]
        if missing or len(self.grads) != len(params):
            raise VarHipError("PPO.capture: the policy has parameters outside its convolution stacks, trunk and head")

    def static_bytes(self):
        return sum(t.numel() * t.element_size() for t in self.buffers)

    def set_grads(self):
        for p in self.owner.agent.actor_critic.parameters():
            p.grad = self.grads[id(p)]

    def run(self):
        """The minibatch step at the cursor, enqueued on the current stream."""
        o, c = self.owner, self.owner._ctx
        agent, ro, lib, s = o.agent, o.storage, o._ctx.lib, current_stream_handle()
        kind, T, nb, M = o.kind, ro.num_steps, self.nb, self.M
        ws, nbytes = ptr(self.ws), self.ws.numel()
        c.check(lib.var_rollout_move_cursor(c.handle, s, self._segs, len(self._segs), ptr(o._ind), o._ind.numel(), ptr(o._cursor), nb,
                                            ro.num_processes), "var_rollout_move_cursor")
        if kind == 0:
            torch.cat([self.obs["image_feat"], self.obs["robot_pose"]], dim=1, out=self.motor_in)
        for st in self.stacks:
            img = st["image"]
            c.check(lib.var_convstack_fwd_ex(c.handle, s, st["kind"], _table(st["params"]), ptr(img), int(img.dtype == torch.uint8),
                                             img.stride(0), M, ptr(st["feat"]), ptr(st["saved"]), ws, nbytes, o.flags),
                    "var_convstack_fwd_ex")
        occ = self.stacks[0] if kind else None
        image = self.stacks[-1]
        sound, masks = self.obs["goal_sound_feat"], self.mb["masks"]
        c.check(lib.var_trunk_fwd(c.handle, s, kind, _table(self.tp), ptr(image["feat"]), ptr(occ["feat"]) if occ else None,
                                  ptr(self.motor_in), ptr(sound), ptr(self.hxs), ptr(masks), T, nb, ptr(self.value), ptr(self.feats),
                                  ptr(self.h_T), ptr(self.t_saved), ws, nbytes), "var_trunk_fwd")
        clipped = bool(agent.use_clipped_value_loss)
        c.check(lib.var_ppo_head_linear(c.handle, s, agent._kind, ptr(self.feats), ptr(self.lin.weight), ptr(self.lin.bias),
                                        ptr(self.logstd), ptr(self.value), ptr(self.mb["actions"]), ptr(self.mb["action_log_probs"]),
                                        ptr(self.mb["advantages"]), ptr(self.mb["returns"]), ptr(self.mb["value_preds"]) if clipped else None,
                                        self.n, M, float(agent.clip_param), float(agent.value_loss_coef), float(agent.entropy_coef),
                                        int(clipped), ptr(self.head), ptr(self.out), ptr(self.g_features), ptr(self.g_W), ptr(self.g_b),
                                        ptr(self.g_value), ptr(self.g_logstd) if agent._kind == 0 else None, ws, nbytes, ptr(o._stats),
                                        o._stats.shape[0], ptr(o._cursor), nb), "var_ppo_head_linear")
        c.check(lib.var_trunk_bwd(c.handle, s, kind, _table(self.tp), ptr(image["feat"]), ptr(occ["feat"]) if occ else None,
                                  ptr(self.motor_in), ptr(sound), ptr(masks), T, nb, ptr(self.t_saved), ptr(self.g_value),
                                  ptr(self.g_features), None, ptr(image["d_feat"]), ptr(occ["d_feat"]) if occ else None, ptr(self.d_hxs),
                                  ptr(self.t_g), ws, nbytes), "var_trunk_bwd")
        for st in self.stacks:
            img = st["image"]
            c.check(lib.var_convstack_bwd_ex(c.handle, s, st["kind"], _table(st["params"]), ptr(img), int(img.dtype == torch.uint8),
                                             img.stride(0), M, ptr(st["saved"]), ptr(st["d_feat"]), ptr(st["g"]), ws, nbytes, None, o.flags),
                    "var_convstack_bwd_ex")
        self.set_grads()
        agent.optimizer.step()


class UpdateStep:
    """PPO.capture(rollouts): see the module docstring.  update(rollouts) is PPO.update's body for the captured storage;
    run_eager(rollouts) runs the same launch sequences without a graph.  n_graphs, static_bytes() and buffer_addresses() describe
    what is held."""

    def __init__(self, agent, rollouts, precision=None):
        pol = agent.actor_critic
        base = getattr(pol, "base", None)
        if base is None or getattr(getattr(base, "forward", None), "__func__", None) is not _convs_forward:
            raise VarHipError("PPO.capture: the policy must be bound with bind_convs (the captured step calls the stacks' and the "
                              "trunk's entries directly)")
        if not agent.fused_optimizer or not agent.fused_head:
            raise VarHipError("PPO.capture: build the agent with fused_optimizer=True and fused_head=True (the captured step is "
                              "their launch sequence)")
        if not isinstance(rollouts, RolloutStorage):
            raise VarHipError("PPO.capture: the rollouts must be var_amd's device-resident RolloutStorage (no CPU fallback)")
        self.flags = _flags(base._convs_precision if precision is None else precision, "PPO.capture")
        self.precision = {v: k for k, v in PRECISIONS.items()}[self.flags]
        self.agent, self.storage, self.device = agent, rollouts, rollouts.device
        self.kind = trunk_kind(base)
        params = list(pol.parameters())
        if any(p.device != self.device or p.dtype != torch.float32 for p in params):
            raise VarHipError(f"PPO.capture: the policy's parameters must be float32 on {self.device}")
        self._arena = [p.data_ptr() for p in params]
        self._ctx = Context.get(self.device.index)
        T, N, mb = rollouts.num_steps, rollouts.num_processes, int(agent.num_mini_batch)
        if N < mb:
            raise VarHipError(f"PPO.capture: {N} processes for {mb} minibatches (recurrent_generator needs N >= num_mini_batch)")
        per = N // mb
        self._shape = (T, N, mb, int(agent.ppo_epoch), tuple(k for k, _, _ in rollouts._obs_items()))
        self._sequence = [min(per, N - start) for start in range(0, N, per)]          # recurrent_generator's minibatches of an epoch
        n_rows = len(self._sequence) * int(agent.ppo_epoch)
        self._ind = torch.zeros(N * int(agent.ppo_epoch), dtype=torch.int32, device=self.device)
        self._perm_host = torch.zeros(N * int(agent.ppo_epoch), dtype=torch.int32).pin_memory()
        self._cursor = torch.zeros(2, dtype=torch.int32, device=self.device)
        self._stats = torch.zeros(n_rows, 3, dtype=torch.float32, device=self.device)
        self._write_lr()
        self._steps = {nb: _Minibatch(self, nb) for nb in sorted(set(self._sequence), reverse=True)}
        before = [p.grad for p in params]
        try:                                                     # (ClipAdam.step's host side runs here: every parameter is active)
            replays = self._ctx.capture([[st.run] for st in self._steps.values()])
        finally:
            for p, g in zip(params, before):
                p.grad = g
        self._replays = dict(zip(self._steps, replays))
        self.n_graphs = len(self._replays)

    def _write_lr(self):
        opt = self.agent.optimizer
        lr = float(opt.param_groups[0]["lr"])
        if lr != opt._lr_written:
            opt._lr_dev.fill_(lr)                                # (a launch, stream-ordered in front of the replays, as ClipAdam.step's)
            opt._lr_written = lr

    def static_bytes(self):
        """Device bytes the static buffers of all graphs hold (the storage and the optimiser's state are not counted)."""
        own = sum(t.numel() * t.element_size() for t in (self._ind, self._cursor, self._stats))
        return own + sum(st.static_bytes() for st in self._steps.values())

    def buffer_addresses(self):
        return tuple(t.data_ptr() for st in self._steps.values() for t in st.buffers) + (self._ind.data_ptr(), self._cursor.data_ptr(),
                                                                                         self._stats.data_ptr())

    def _check(self, rollouts):
        agent = self.agent
        if rollouts is not self.storage:
            same = isinstance(rollouts, RolloutStorage) and (rollouts.num_steps, rollouts.num_processes) == self._shape[:2]
            raise VarHipError("UpdateStep: captured for another storage" + ("" if same else " (another (T, N) or no RolloutStorage)") +
                              ": the graphs read the captured storage's tensors in place; call PPO.capture(rollouts) for this one")
        shape = (rollouts.num_steps, rollouts.num_processes, int(agent.num_mini_batch), int(agent.ppo_epoch),
                 tuple(k for k, _, _ in rollouts._obs_items()))
        if shape != self._shape:
            raise VarHipError(f"UpdateStep: (T, N, num_mini_batch, ppo_epoch, obs keys) {shape} differ from the captured {self._shape}: "
                              "call PPO.capture again")
        held = [t.data_ptr() for st in self._steps.values() for t in st._held]
        now = [t.data_ptr() for st in self._steps.values() for t in
               [store for _, store, _ in rollouts._obs_items()] + [rollouts.actions, rollouts.value_preds, rollouts.returns, rollouts.masks,
                                                                   rollouts.action_log_probs, rollouts._advantages,
                                                                   rollouts.recurrent_hidden_states]]
        if held != now:
            raise VarHipError("UpdateStep: the storage's tensors have been replaced since PPO.capture: call it again")
        if [p.data_ptr() for p in agent.actor_critic.parameters()] != self._arena:
            raise VarHipError("UpdateStep: the policy's parameter arena has moved since PPO.capture (.to(), re-flattened parameters): "
                              "call PPO.capture again")
        if not agent.fused_optimizer or not agent.fused_head:
            raise VarHipError("UpdateStep: the agent's fused_optimizer / fused_head have been switched off since PPO.capture")
        rollouts.advantages()                                    # (raises without compute_returns)

    def update(self, rollouts, _eager=False):
        """PPO.update for the captured storage: (value_loss, action_loss, dist_entropy) averaged as the eager update averages."""
        self._check(rollouts)
        agent = self.agent
        N, epochs = rollouts.num_processes, int(agent.ppo_epoch)
        for e in range(epochs):
            self._perm_host[e * N:(e + 1) * N] = torch.randperm(N).to(torch.int32)     # where recurrent_generator draws it
        self._ind.copy_(self._perm_host, non_blocking=True)
        self._cursor.fill_(0)
        self._write_lr()
        last = None
        for _ in range(epochs):
            for nb in self._sequence:
                last = self._steps[nb]
                if _eager:
                    last.run()
                else:
                    self._replays[nb]()
        last.set_grads()
        num_updates = agent.ppo_epoch * agent.num_mini_batch
        sums = self._stats.sum(0).tolist()                       # (the one host read of an update)
        return sums[0] / num_updates, sums[1] / num_updates, sums[2] / num_updates

    def run_eager(self, rollouts):
        """update() with every minibatch step enqueued launch by launch instead of replayed."""
        return self.update(rollouts, _eager=True)

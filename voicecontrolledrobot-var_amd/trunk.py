"""The PPO update's MLP trunk (csrc/trunk.hip; include/var_hip.h: var_trunk_fwd / var_trunk_bwd): everything between imgCNN's
flattened output and the distribution head of armNet_VAR (models/RL/arm_RL_model.py:102-134) and ai2thorNet_VAR
(models/RL/ai2thor_RL_model.py:85-115) -- the 20 | 21 Linear + ReLU layers, the three residual sums and the masked GRU of
gru_seq.py in the middle -- forward and backward, as one autograd node.

    value, actor_features, h_T = trunk_eval(base, feat, motor_in, sound_in, hxs, masks, occ=None)
    ppo = PPO(bind_trunk(policy), ...)        # policy.base(obs, hxs, masks) now runs imgCNN in PyTorch, then trunk_eval

bind_trunk works on the reference's Policy and on ArmNetPolicy / IthorNetPolicy alike: with it var_amd.PPO trains the very
object whose capture() acts (Adam -- PyTorch's, or var_amd.ClipAdam with PPO(..., fused_optimizer=True) -- updates the arena in
place; the acting graph re-packs per replay).  With bind_trunk the
convolution stacks' evaluation stays in PyTorch autograd; convstack.py's bind_convs puts them into HIP as well
(conv_stack_eval), and then nothing of the base's evaluation is left to PyTorch autograd kernels.  GPU only, fp32 only: there is no CPU fallback, anything else raises VarHipError
before a launch.  Nothing here reads the device, so the op can sit inside a torch.cuda.graph capture."""
import ctypes
import types

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from ._lib import Context, VarHipError, current_stream_handle, load_library, ptr

# per kind: (H, motor_in's width, the Sequentials in state_dict order with the indices of their trunk Linear layers)
_LAYOUT = {
    0: (512, 5, (("motorMlp", (0, 2, 4)), ("cnnMlp", (0, 2)), ("imgMotorMlp", (0, 2)), ("imgMotorMlp2", (0,)),
                 ("soundMlp", (0, 2, 4)), ("fusionMlp", (0, 2)), ("mlp_all", (0, 2)), ("actor", (0, 2)), ("critic", (0, 2)))),
    1: (1024, 3, (("occupancyCNNMLP", (5, 7)), ("motorMlp", (0, 2)), ("cnnMlp", (0, 2)), ("imgMotorMlp", (0, 2)),
                  ("imgMotorMlp2", (0,)), ("soundMlp", (0, 2, 4)), ("fusionMlp", (0, 2)), ("mlp_all", (0, 2)), ("actor", (0, 2)),
                  ("critic", (0, 2)))),
}


def trunk_kind(base):
    """0 (arm_VAR) or 1 (ai2thor_VAR), from the base's layer shapes; anything else raises VarHipError."""
    gru = getattr(base, "gru", None)
    if not isinstance(gru, nn.GRU) or gru.num_layers != 1 or gru.bidirectional or not gru.bias or gru.input_size != 128:
        raise VarHipError("trunk: the base needs the reference's one-layer nn.GRU over 128 inputs (a recurrent armNet_VAR / ai2thorNet_VAR)")
    kind = {512: 0, 1024: 1}.get(gru.hidden_size)
    if kind is None or (kind == 1) != hasattr(base, "occupancyCNNMLP"):
        raise VarHipError(f"trunk: recurrent size {gru.hidden_size} is neither arm_VAR's Kuka configuration (512) nor ai2thor_VAR's (1024, "
                          "with occupancyCNNMLP)")
    return kind


def trunk_param_names(kind):
    """The published parameter order (var_trunk_param_floats): names relative to the base."""
    names = ["gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0"]
    for seq, idx in _LAYOUT[kind][2]:
        for i in idx:
            names += [f"{seq}.{i}.weight", f"{seq}.{i}.bias"]
    return names + ["critic_linear.weight", "critic_linear.bias"]


def trunk_layer_names(kind):
    """The trunk's Linear layers in the published order ('motorMlp.0', ...): the keys of the saved-activation map."""
    return [n[:-len(".weight")] for n in trunk_param_names(kind)[4:] if n.endswith(".weight")]


def trunk_parameters(base, kind=None):
    """The base's trunk parameters in the published order, shapes checked against the library's."""
    kind = trunk_kind(base) if kind is None else kind
    lib = load_library()
    names = trunk_param_names(kind)
    if lib.var_trunk_n_params(kind) != len(names):
        raise VarHipError("trunk: the library publishes another parameter count")
    params = []
    for i, name in enumerate(names):
        obj = base
        try:
            for part in name.split("."):
                obj = obj[int(part)] if part.isdigit() else getattr(obj, part)
        except (AttributeError, IndexError, TypeError):
            raise VarHipError(f"trunk: the base has no parameter {name}") from None
        if not torch.is_tensor(obj) or obj.numel() != lib.var_trunk_param_floats(kind, i):
            raise VarHipError(f"trunk: {name} has {getattr(obj, 'shape', None)}, the kind-{kind} trunk holds "
                              f"{lib.var_trunk_param_floats(kind, i)} floats there")
        params.append(obj)
    return params


def _check_inputs(kind, feat, motor_in, sound_in, hxs, masks, occ, params):
    H, nm, _ = _LAYOUT[kind]
    named = [("feat", feat), ("motor_in", motor_in), ("sound_in", sound_in), ("hxs", hxs), ("masks", masks)]
    if kind == 1:
        if occ is None:
            raise VarHipError("trunk_eval: the ai2thor_VAR trunk needs occ (M, 288)")
        named.append(("occ", occ))
    elif occ is not None:
        raise VarHipError("trunk_eval: the arm_VAR trunk has no occupancy branch")
    for name, t in named + [("a parameter", p) for p in params]:
        if not torch.is_tensor(t):
            raise VarHipError(f"trunk_eval: {name} must be a tensor")
        if not t.is_cuda:
            raise VarHipError(f"trunk_eval: {name} is on {t.device}: inputs must be CUDA tensors (no CPU fallback)")
        if t.device != feat.device:
            raise VarHipError(f"trunk_eval: {name} is on {t.device}, feat on {feat.device}")
        if t.dtype != torch.float32:
            raise VarHipError(f"trunk_eval: {name} is {t.dtype}, float32 only")
    if hxs.dim() != 2 or hxs.shape[1] != H or not 1 <= hxs.shape[0] <= 64:
        raise VarHipError(f"trunk_eval: hxs must be (N, {H}) with N in 1..64, got {tuple(hxs.shape)}")
    N, M = hxs.shape[0], feat.shape[0] if feat.dim() == 2 else -1
    if M < N or M % N:
        raise VarHipError(f"trunk_eval: feat {tuple(feat.shape)} for N = {N} environments (rows = T*N, T >= 1)")
    for name, t, cols in (("feat", feat, 1152), ("motor_in", motor_in, nm), ("sound_in", sound_in, 3), ("occ", occ, 288)):
        if t is not None and tuple(t.shape) != (M, cols):
            raise VarHipError(f"trunk_eval: {name} must be ({M}, {cols}), got {tuple(t.shape)}")
    if masks.numel() != M or masks.dim() not in (1, 2) or (masks.dim() == 2 and masks.shape[1] != 1):
        raise VarHipError(f"trunk_eval: masks must be ({M}, 1), got {tuple(masks.shape)}")
    return M // N, N, H


def _pointer_table(tensors):
    return (ctypes.c_void_p * len(tensors))(*(t.data_ptr() for t in tensors))


def _workspace(c, kind, T, N, dev):
    nbytes = c.lib.var_trunk_workspace_bytes(kind, T, N)
    if nbytes < 0:
        raise VarHipError(f"var_trunk_workspace_bytes refused kind {kind}, T {T}, N {N}")
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev), int(nbytes)


class _Trunk(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, keep, feat, motor_in, sound_in, hxs, masks, occ, *params):
        T, N, H = _check_inputs(kind, feat, motor_in, sound_in, hxs, masks, occ, params)
        dev, M = feat.device, T * N
        ins = [t.detach().contiguous() for t in (feat, motor_in, sound_in, hxs, masks)]
        oc = occ.detach().contiguous() if occ is not None else None
        ps = [p.detach().contiguous() for p in params]
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # noqa: E731
        value, feats, h_T = new(M, 1), new(M, 128), new(N, H)
        c = Context.get(dev.index)
        need = keep or any(ctx.needs_input_grad)
        saved = new(c.lib.var_trunk_saved_floats(kind, T, N)) if need else None
        ws, nbytes = _workspace(c, kind, T, N, dev)
        c.check(c.lib.var_trunk_fwd(c.handle, current_stream_handle(), kind, _pointer_table(ps), ptr(ins[0]), ptr(oc), ptr(ins[1]),
                                    ptr(ins[2]), ptr(ins[3]), ptr(ins[4]), T, N, ptr(value), ptr(feats), ptr(h_T), ptr(saved),
                                    ptr(ws), nbytes),
                "var_trunk_fwd")
        if need:
            ctx.save_for_backward(ins[0], ins[1], ins[2], ins[4], saved, *([oc] if oc is not None else []), *ps)
        ctx.dims = (kind, T, N, H, oc is not None)
        ctx.set_materialize_grads(False)
        if keep:
            ctx.mark_non_differentiable(saved)
            return value, feats, h_T, saved
        return value, feats, h_T

    @staticmethod
    @once_differentiable
    def backward(ctx, d_value, d_feats, d_hT, *_):
        kind, T, N, H, has_occ = ctx.dims
        feat, motor_in, sound_in, masks, saved, *rest = ctx.saved_tensors
        oc = rest.pop(0) if has_occ else None
        ps = rest
        dev, M = feat.device, T * N
        d_value, d_feats, d_hT = (None if g is None else g.contiguous() for g in (d_value, d_feats, d_hT))
        c = Context.get(dev.index)
        lib = c.lib
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # noqa: E731
        d_feat, d_hxs = new(M, 1152), new(N, H)
        d_occ = new(M, 288) if has_occ else None
        n = len(ps)
        offs = [lib.var_trunk_grad_offset(kind, i) for i in range(n + 1)]
        flat = new(offs[n])
        ws, nbytes = _workspace(c, kind, T, N, dev)
        c.check(lib.var_trunk_bwd(c.handle, current_stream_handle(), kind, _pointer_table(ps), ptr(feat), ptr(oc), ptr(motor_in),
                                  ptr(sound_in), ptr(masks), T, N, ptr(saved), ptr(d_value), ptr(d_feats), ptr(d_hT), ptr(d_feat),
                                  ptr(d_occ), ptr(d_hxs), ptr(flat), ptr(ws), nbytes),
                "var_trunk_bwd")
        grads = tuple(flat[offs[i]:offs[i] + p.numel()].view(p.shape) for i, p in enumerate(ps))   # views of the one buffer
        return (None, None, d_feat, None, None, d_hxs, None, d_occ) + grads


def saved_map(kind, T, N):
    """name -> (offset, rows, columns) into the flat `saved` tensor: every trunk layer's activation under its layer name
    ('motorMlp.0', ...), 'gru' (the GRU's output, (M, H)) and 'gru.saved' (var_gru_seq_fwd's r | z | n | gh_n | h', (5 M, H))."""
    lib = load_library()
    H, M, names = _LAYOUT[kind][0], T * N, trunk_layer_names(kind)
    m = {}
    for i, name in enumerate(names):
        m[name] = (lib.var_trunk_saved_offset(kind, T, N, i), M, lib.var_trunk_param_floats(kind, 5 + 2 * i))
    m["gru"] = (lib.var_trunk_saved_offset(kind, T, N, len(names)), M, H)
    m["gru.saved"] = (lib.var_trunk_saved_offset(kind, T, N, len(names) + 1), 5 * M, H)
    return m


def trunk_eval(base, feat, motor_in, sound_in, hxs, masks, occ=None, return_saved=False):
    """feat (M, 1152) = imgCNN's flattened output, motor_in (M, 5 | 3), sound_in (M, 3), hxs (N, H), masks (M, 1), occ (M, 288:
    ai2thor_VAR only, occupancyCNNMLP's flattened convolution output) -> (value (M, 1), actor_features (M, 128), h_T (N, H)); M =
    T*N rows ordered (t, n).  Differentiable in feat, occ, hxs and every trunk parameter of `base` (their gradients are views of
    one flat buffer); motor_in, sound_in and masks carry no gradient.  return_saved: also (saved, map) -- the flat tensor of
    saved activations and saved_map's name -> (offset, rows, columns)."""
    kind = trunk_kind(base)
    params = trunk_parameters(base, kind)
    out = _Trunk.apply(kind, bool(return_saved), feat, motor_in, sound_in, hxs, masks, occ, *params)
    if return_saved:
        T = feat.shape[0] // hxs.shape[0]
        return out[0], out[1], out[2], out[3], saved_map(kind, T, hxs.shape[0])
    return out


def _image(t):
    return t.float() / 255.0 if t.dtype == torch.uint8 else t.float()


def _trunk_forward(self, inputs, rnn_hxs, masks, **kw):
    """armNet_VAR.forward / ai2thorNet_VAR.forward: imgCNN (and the occupancy convolutions) in PyTorch, the rest in trunk_eval."""
    kind = trunk_kind(self)
    image = _image(inputs['image'])
    if kind == 0:
        motor_in = torch.cat([inputs['image_feat'].float(), inputs['robot_pose'].float()], dim=1)
        occ = None
    else:
        motor_in = inputs['image_feat'].float()
        occ = _image(inputs['occupancy'])
        for mod in list(self.occupancyCNNMLP)[:5]:
            occ = mod(occ)
    feat = self.imgCNN(image)
    value, feats, h_T = trunk_eval(self, feat, motor_in, inputs['goal_sound_feat'].float(), rnn_hxs, masks, occ=occ)
    return value, feats, h_T, {}


def bind_trunk(policy):
    """Give policy.base (the reference's Policy, ArmNetPolicy, IthorNetPolicy: anything whose base holds the trunk's modules) a
    forward(inputs, rnn_hxs, masks, **kw) -> (value, actor_features, rnn_hxs, {}) over trunk_eval; returns the policy, so that
    PPO(bind_trunk(policy), ...) reads like bind_forward_gru."""
    base = getattr(policy, "base", None)
    if base is None:
        raise VarHipError("bind_trunk: the policy has no .base")
    kind = trunk_kind(base)
    trunk_parameters(base, kind)
    if not isinstance(getattr(base, "imgCNN", None), nn.Module):
        raise VarHipError("bind_trunk: the base has no imgCNN module")
    base.forward = types.MethodType(_trunk_forward, base)
    return policy

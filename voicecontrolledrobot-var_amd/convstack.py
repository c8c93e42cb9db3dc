"""The actor-critics' convolution stacks (csrc/convstack.hip; include/var_hip.h: var_convstack_fwd / var_convstack_bwd):
armNet_VAR.imgCNN's 96 x 96 branch (kind 0, models/RL/arm_RL_model.py:22-34), ai2thorNet_VAR.imgCNN (kind 1,
models/RL/ai2thor_RL_model.py:16-25) and the two convolutions of occupancyCNNMLP (kind 2, :34-35), forward and backward, as one
autograd node.

    feat = conv_stack_eval(base.imgCNN, image)           # (B, 1152); image uint8 (divided by 255 on the device) or float32
    ppo = PPO(bind_convs(policy), ...)                   # policy.base(obs, hxs, masks): conv_stack_eval, then trunk_eval
    ppo = PPO(bind_convs(policy, precision="bf16"), ...) # the same with the stacks' products on bf16 operands

precision="bf16" (flags bit 0 of var_convstack_fwd_ex / _bwd_ex; include/var_hip.h has the definition): every convolution product
of kinds 0 and 1, in all three directions, multiplies operands rounded to bf16 and accumulates in fp32; everything stored, every
layout, the parameters, their gradients, the trunk, the optimiser and the acting forwards stay fp32.  Kind 2 computes in fp32
under either name.  Opt-in: without it every entry gives the bits it gave before the mode existed.

bind_convs works on the reference's Policy and on ArmNetPolicy / IthorNetPolicy alike; with it the whole base is evaluated, forward
and backward, without a PyTorch autograd kernel and without MIOpen (PPO(..., fused_optimizer=True) takes the gradient clip and
Adam from PyTorch's kernels as well: optim.py).  The op differentiates in the parameters only: the
observations carry no gradient in PPO.  GPU only, fp32 tensors only: there is no CPU fallback, anything else raises VarHipError before a
launch.  Nothing here reads the device, so the op can sit inside a torch.cuda.graph capture."""
import ctypes
import types

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from ._lib import Context, VarHipError, current_stream_handle, load_library, ptr
from .trunk import trunk_eval, trunk_kind, trunk_parameters

# per kind: input (C, H, W), then per convolution (in, out, stride, padding, a MaxPool2d(2, 2) follows)
_STACKS = {
    0: ((3, 96, 96), ((3, 32, 1, 1, False), (32, 32, 1, 1, True), (32, 64, 1, 1, False), (64, 64, 1, 1, True), (64, 128, 1, 1, False),
                      (128, 128, 1, 1, True), (128, 256, 2, 0, False), (256, 128, 1, 0, False))),
    1: ((3, 96, 96), ((3, 32, 1, 1, False), (32, 32, 1, 1, True), (32, 64, 1, 1, True), (64, 64, 1, 1, True), (64, 128, 1, 1, True),
                      (128, 128, 2, 1, False))),
    2: ((1, 9, 9), ((1, 64, 2, 1, False), (64, 32, 2, 1, False))),
}
MAX_BATCH = 1024
PRECISIONS = {"fp32": 0, "bf16": 1}                      # name -> flags of the _ex entries


def _flags(precision, who):
    if precision not in PRECISIONS:
        raise VarHipError(f"{who}: precision {precision!r} is neither 'fp32' nor 'bf16'")
    return PRECISIONS[precision]


def _pair(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


def _signature(mods):
    """(in, out, stride, padding, pooled) per convolution of a module list, or None where it is not conv + ReLU (+ pool) throughout."""
    sig, i = [], 0
    while i < len(mods):
        m = mods[i]
        if not isinstance(m, nn.Conv2d) or i + 1 >= len(mods) or not isinstance(mods[i + 1], nn.ReLU):
            return None
        if (_pair(m.kernel_size) != (3, 3) or _pair(m.dilation) != (1, 1) or m.groups != 1 or m.bias is None or m.padding_mode != "zeros"
                or _pair(m.stride)[0] != _pair(m.stride)[1] or not isinstance(m.padding, (tuple, list, int))
                or _pair(m.padding)[0] != _pair(m.padding)[1]):
            return None
        i += 2
        pooled = False
        if i < len(mods) and isinstance(mods[i], nn.MaxPool2d):
            p = mods[i]
            if (_pair(p.kernel_size) != (2, 2) or _pair(p.stride) != (2, 2) or _pair(p.padding) != (0, 0) or _pair(p.dilation) != (1, 1)
                    or p.ceil_mode):
                return None
            pooled, i = True, i + 1
        sig.append((m.in_channels, m.out_channels, _pair(m.stride)[0], _pair(m.padding)[0], pooled))
    return tuple(sig)


def _conv_part(module):
    """The convolution part of imgCNN (everything before Flatten) or of occupancyCNNMLP (everything before its Flatten)."""
    if not isinstance(module, nn.Sequential):
        raise VarHipError("conv_stack: the module must be the reference's nn.Sequential (imgCNN or occupancyCNNMLP)")
    mods = list(module)
    for i, m in enumerate(mods):
        if isinstance(m, nn.Flatten) or type(m).__name__ == "Flatten":
            return mods[:i]
    raise VarHipError("conv_stack: the module has no Flatten after its convolutions")


def stack_kind(module):
    """0 (arm_VAR imgCNN, 96 x 96 branch), 1 (ai2thor_VAR imgCNN) or 2 (occupancyCNNMLP's convolutions), from the module's layers;
    anything else -- buildCNN's 7 x 7 branch for 120 x 160 images among it -- raises VarHipError."""
    sig = _signature(_conv_part(module))
    for kind, (_, want) in _STACKS.items():
        if sig == want:
            return kind
    raise VarHipError("conv_stack: the module is none of armNet_VAR.imgCNN (96 x 96 branch), ai2thorNet_VAR.imgCNN and "
                      "occupancyCNNMLP; buildCNN's 7 x 7 branch for 120 x 160 images is not implemented")


def stack_param_names(kind):
    """The published parameter order (var_convstack_param_floats): names relative to the Sequential ('0.weight', '0.bias', ...)."""
    idx, i = [], 0
    for (_, _, _, _, pooled) in _STACKS[kind][1]:
        idx.append(i)
        i += 3 if pooled else 2
    return [f"{j}.{w}" for j in idx for w in ("weight", "bias")]


def stack_parameters(module, kind=None):
    """The module's convolution parameters in the published order, shapes checked against the library's."""
    kind = stack_kind(module) if kind is None else kind
    lib = load_library()
    names = stack_param_names(kind)
    if lib.var_convstack_n_params(kind) != len(names):
        raise VarHipError("conv_stack: the library publishes another parameter count")
    params = []
    for i, name in enumerate(names):
        j, w = name.split(".")
        p = getattr(module[int(j)], w)
        cin, cout = _STACKS[kind][1][i // 2][:2]
        want = (cout, cin, 3, 3) if w == "weight" else (cout,)
        if tuple(p.shape) != want or p.numel() != lib.var_convstack_param_floats(kind, i):
            raise VarHipError(f"conv_stack: {name} has {tuple(p.shape)}, the kind-{kind} stack holds {want} there")
        params.append(p)
    return params


def saved_map(kind, B):
    """name -> (offset, shape) into the flat `saved` tensor: every convolution's post-ReLU map (B, C, H, H), un-pooled where a pool
    follows, under its module index in the Sequential ('0', '2', '5', ...)."""
    lib = load_library()
    (_, h, _), convs = _STACKS[kind]
    names = stack_param_names(kind)[::2]
    m = {}
    for j, (cin, cout, stride, pad, pooled) in enumerate(convs):
        h = (h + 2 * pad - 3) // stride + 1
        m[names[j][:-len(".weight")]] = (lib.var_convstack_saved_offset(kind, B, j), (B, cout, h, h))
        h = h // 2 if pooled else h
    return m


def _check(kind, image, params):
    (C, H, W), convs = _STACKS[kind]
    if not torch.is_tensor(image):
        raise VarHipError("conv_stack_eval: the image must be a tensor")
    for name, t in [("the image", image)] + [("a parameter", p) for p in params]:
        if not t.is_cuda:
            raise VarHipError(f"conv_stack_eval: {name} is on {t.device}: inputs must be CUDA tensors (no CPU fallback)")
        if t.device != image.device:
            raise VarHipError(f"conv_stack_eval: {name} is on {t.device}, the image on {image.device}")
    if image.dtype not in (torch.uint8, torch.float32):
        raise VarHipError(f"conv_stack_eval: the image is {image.dtype}: uint8 (divided by 255 on the device) or float32")
    for p in params:
        if p.dtype != torch.float32:
            raise VarHipError(f"conv_stack_eval: a parameter is {p.dtype}, float32 only")
    if image.dim() != 4 or tuple(image.shape[1:]) != (C, H, W):
        raise VarHipError(f"conv_stack_eval: the kind-{kind} stack takes (B, {C}, {H}, {W}), got {tuple(image.shape)}")
    if not 1 <= image.shape[0] <= MAX_BATCH:
        raise VarHipError(f"conv_stack_eval: B = {image.shape[0]} is outside 1..{MAX_BATCH}")
    if image.requires_grad:
        raise VarHipError("conv_stack_eval: the image requires grad, but the op has no image gradient (observations carry none in PPO)")
    return int(image.shape[0]), convs[-1][1] * 9


def _pointer_table(tensors):
    return (ctypes.c_void_p * len(tensors))(*(t.data_ptr() for t in tensors))


def _workspace(c, kind, B, dev, flags):
    nbytes = c.lib.var_convstack_workspace_bytes_ex(kind, B, flags)
    if nbytes < 0:
        raise VarHipError(f"var_convstack_workspace_bytes_ex refused kind {kind}, B {B}, flags {flags}")
    return torch.empty(int(nbytes), dtype=torch.uint8, device=dev), int(nbytes)


class _ConvStack(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, keep, flags, grad_maps, image, *params):
        B, nfeat = _check(kind, image, params)
        dev = image.device
        img = image.detach().contiguous()
        ps = [p.detach().contiguous() for p in params]
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # noqa: E731
        c = Context.get(dev.index)
        feat = new(B, nfeat)
        need = keep or any(ctx.needs_input_grad)
        saved = new(c.lib.var_convstack_saved_floats(kind, B)) if need else None
        if grad_maps is not None:
            n = c.lib.var_convstack_saved_floats(kind, B)
            if (not torch.is_tensor(grad_maps) or grad_maps.dtype != torch.float32 or grad_maps.device != dev or grad_maps.dim() != 1
                    or grad_maps.numel() != n or not grad_maps.is_contiguous() or grad_maps.requires_grad):
                raise VarHipError(f"conv_stack_eval: grad_maps must be a contiguous float32 tensor of {n} elements (saved's length) on "
                                  f"{dev} that requires no grad")
        ws, nbytes = _workspace(c, kind, B, dev, flags)
        u8 = int(img.dtype == torch.uint8)
        c.check(c.lib.var_convstack_fwd_ex(c.handle, current_stream_handle(), kind, _pointer_table(ps), ptr(img), u8, img.stride(0), B,
                                           ptr(feat), ptr(saved), ptr(ws), nbytes, flags),
                "var_convstack_fwd_ex")
        if need:
            ctx.save_for_backward(img, saved, *ps)
        ctx.dims = (kind, B, u8, flags)
        ctx.grad_maps = grad_maps
        ctx.set_materialize_grads(False)
        if keep:
            ctx.mark_non_differentiable(saved)
            return feat, saved
        return feat

    @staticmethod
    @once_differentiable
    def backward(ctx, d_feat, *_):
        kind, B, u8, flags = ctx.dims
        img, saved, *ps = ctx.saved_tensors
        if d_feat is None:
            return (None,) * (5 + len(ps))
        dev = img.device
        d_feat = d_feat.contiguous()
        c = Context.get(dev.index)
        lib = c.lib
        n = len(ps)
        offs = [lib.var_convstack_grad_offset(kind, i) for i in range(n + 1)]
        flat = torch.empty(offs[n], dtype=torch.float32, device=dev)
        ws, nbytes = _workspace(c, kind, B, dev, flags)
        c.check(lib.var_convstack_bwd_ex(c.handle, current_stream_handle(), kind, _pointer_table(ps), ptr(img), u8, img.stride(0), B,
                                         ptr(saved), ptr(d_feat), ptr(flat), ptr(ws), nbytes, ptr(ctx.grad_maps), flags),
                "var_convstack_bwd_ex")
        grads = tuple(flat[offs[i]:offs[i] + p.numel()].view(p.shape) for i, p in enumerate(ps))   # views of the one buffer
        return (None,) * 5 + grads


def conv_stack_eval(module, image, return_saved=False, precision="fp32", grad_maps=None):
    """module: armNet_VAR.imgCNN (96 x 96 branch), ai2thorNet_VAR.imgCNN or occupancyCNNMLP (its two convolutions are evaluated,
    the Linear layers behind its Flatten belong to trunk_eval); image (B, 3, 96, 96) | (B, 1, 9, 9), uint8 (divided by 255 on the
    device) or float32 -> feat (B, 1152 | 288), the last map flattened.  Differentiable in the module's convolution parameters
    (their gradients are views of one flat buffer), not in the image.  return_saved: also (saved, map) -- the flat tensor of
    saved activations and saved_map's name -> (offset, shape).  precision: "fp32", or "bf16" for products on operands rounded
    to bf16 (the module docstring; kind 2 computes in fp32 either way); anything else raises VarHipError before the device is
    touched.  grad_maps: a float32 CUDA tensor of `saved`'s length and layout that the backward fills with every convolution's
    gated gradient map g_l (the gradient with respect to its un-pooled pre-activation), in either precision; the parameter
    gradients have the same bits with and without it."""
    flags = _flags(precision, "conv_stack_eval")
    kind = stack_kind(module)
    params = stack_parameters(module, kind)
    out = _ConvStack.apply(kind, bool(return_saved), flags, grad_maps, image, *params)
    if return_saved:
        return out[0], out[1], saved_map(kind, image.shape[0])
    return out


def _as_image(t):
    return t if t.dtype == torch.uint8 else t.float()


def _convs_forward(self, inputs, rnn_hxs, masks, **kw):
    """armNet_VAR.forward / ai2thorNet_VAR.forward: the convolutions in conv_stack_eval, the rest in trunk_eval."""
    kind = trunk_kind(self)
    if kind == 0:
        motor_in = torch.cat([inputs['image_feat'].float(), inputs['robot_pose'].float()], dim=1)
        occ = None
    else:
        motor_in = inputs['image_feat'].float()
        occ = conv_stack_eval(self.occupancyCNNMLP, _as_image(inputs['occupancy']), precision=self._convs_precision)
    feat = conv_stack_eval(self.imgCNN, _as_image(inputs['image']), precision=self._convs_precision)
    value, feats, h_T = trunk_eval(self, feat, motor_in, inputs['goal_sound_feat'].float(), rnn_hxs, masks, occ=occ)
    return value, feats, h_T, {}


def bind_convs(policy, precision="fp32"):
    """Give policy.base (the reference's Policy, ArmNetPolicy, IthorNetPolicy) a forward(inputs, rnn_hxs, masks, **kw) -> (value,
    actor_features, rnn_hxs, {}) that runs imgCNN (and, for ai2thor_VAR, occupancyCNNMLP's two convolutions) through
    conv_stack_eval and everything behind them through trunk_eval; returns the policy, so that PPO(bind_convs(policy), ...) reads
    like bind_trunk.  precision: conv_stack_eval's, for the stacks alone -- the trunk, the head, the parameters, their gradients and
    the acting forwards stay fp32, so with "bf16" the importance ratio of the first minibatch after a rollout is close to 1, not 1.
    The matching acting setting is policy.set_acting_precision("bf16"): the acting forwards then round where this evaluation does."""
    _flags(precision, "bind_convs")
    base = getattr(policy, "base", None)
    if base is None:
        raise VarHipError("bind_convs: the policy has no .base")
    kind = trunk_kind(base)
    trunk_parameters(base, kind)
    if not isinstance(getattr(base, "imgCNN", None), nn.Module):
        raise VarHipError("bind_convs: the base has no imgCNN module")
    if stack_kind(base.imgCNN) != kind:
        raise VarHipError("bind_convs: imgCNN is not the stack of the base's kind")
    stack_parameters(base.imgCNN, kind)
    if kind == 1:
        if stack_kind(base.occupancyCNNMLP) != 2:
            raise VarHipError("bind_convs: occupancyCNNMLP does not start with the reference's two convolutions")
        stack_parameters(base.occupancyCNNMLP, 2)
    base._convs_precision = precision
    base.forward = types.MethodType(_convs_forward, base)
    return policy

"""The PPO update's recurrent sequence (csrc/gru_seq.hip; include/var_hip.h: var_gru_seq_fwd / var_gru_seq_bwd): the masked
GRU of the reference's NNBase._forward_gru (models/ppo/model.py:116-171), forward and backward, without the host read of the
zero-mask steps, the per-segment nn.GRU calls and the torch.cat.

    out, h_T = masked_gru(x, hxs, masks, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0)
    x, hxs = forward_gru(base.gru, x, hxs, masks)          # NNBase._forward_gru's signature and return, both branches
    bind_forward_gru(policy)                               # policy.base._forward_gru now runs it

For t = 0..T-1 with h_{-1} = hxs: h' = h_{t-1} * m_t, then one nn.GRU cell step from h' on x_t.  For 0/1 masks that is the
reference's segmented form exactly (it multiplies all rows by masks[t] wherever some row is 0; elsewhere every mask is 1.0);
other mask values are multiplied in as they are, which the reference does not do.  GPU only, fp32 only: there is no CPU
fallback, anything else raises VarHipError before a launch.  Nothing here reads the device, so the op can sit inside a
torch.cuda.graph capture.  trunk.py runs the same entry points inside the whole trunk's forward and backward (bind_trunk)."""
import types

import torch
import torch.nn as nn
from torch.autograd.function import once_differentiable

from ._lib import Context, VarHipError, current_stream_handle, ptr

MAX_H, MAX_I, MAX_N = 1024, 1024, 64


def _check(x, hxs, masks, w_ih, w_hh, b_ih, b_hh):
    """Shapes, dtypes and devices, before anything is loaded or launched; returns (T, N, I, H)."""
    named = (("x", x), ("hxs", hxs), ("masks", masks), ("w_ih", w_ih), ("w_hh", w_hh), ("b_ih", b_ih), ("b_hh", b_hh))
    for name, t in named:
        if not torch.is_tensor(t):
            raise VarHipError(f"masked_gru: {name} must be a tensor")
    for name, t in named:
        if not t.is_cuda:
            raise VarHipError(f"masked_gru: {name} is on {t.device}: inputs must be CUDA tensors (no CPU fallback)")
        if t.device != x.device:
            raise VarHipError(f"masked_gru: {name} is on {t.device}, x on {x.device}")
        if t.dtype != torch.float32:
            raise VarHipError(f"masked_gru: {name} is {t.dtype}, float32 only")
    if x.dim() != 2 or hxs.dim() != 2:
        raise VarHipError(f"masked_gru: x must be (T*N, I) and hxs (N, H), got {tuple(x.shape)} and {tuple(hxs.shape)}")
    N, H = hxs.shape
    rows, I = x.shape
    if N < 1 or N > MAX_N or rows < N or rows % N:
        raise VarHipError(f"masked_gru: {rows} rows of x for N = {N} environments (N in 1..{MAX_N}, rows = T*N, T >= 1)")
    if H < 64 or H > MAX_H or H % 64:
        raise VarHipError(f"masked_gru: H = {H} (a multiple of 64 up to {MAX_H})")
    if I < 1 or I > MAX_I:
        raise VarHipError(f"masked_gru: I = {I} (1..{MAX_I})")
    if masks.numel() != rows or (masks.dim() == 2 and masks.shape != (rows, 1)) or masks.dim() not in (1, 2):
        raise VarHipError(f"masked_gru: masks must be ({rows}, 1), got {tuple(masks.shape)}")
    for name, t, shape in (("w_ih", w_ih, (3 * H, I)), ("w_hh", w_hh, (3 * H, H)), ("b_ih", b_ih, (3 * H,)), ("b_hh", b_hh, (3 * H,))):
        if tuple(t.shape) != shape:
            raise VarHipError(f"masked_gru: {name} must be {shape} (nn.GRU's layout, gates r, z, n), got {tuple(t.shape)}")
    return rows // N, N, I, H


def _workspace(c, T, N, I, H, dev):
    nbytes = c.lib.var_gru_seq_workspace_bytes(T, N, I, H)
    if nbytes < 0:
        raise VarHipError(f"var_gru_seq_workspace_bytes refused T {T}, N {N}, I {I}, H {H}")
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=dev), int(nbytes)


class _MaskedGRU(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, hxs, masks, w_ih, w_hh, b_ih, b_hh):
        T, N, I, H = _check(x, hxs, masks, w_ih, w_hh, b_ih, b_hh)
        dev = x.device
        xs, hs, ms = x.detach().contiguous(), hxs.detach().contiguous(), masks.detach().contiguous()
        wi, wh, bi, bh = (t.detach().contiguous() for t in (w_ih, w_hh, b_ih, b_hh))
        out = torch.empty((T * N, H), dtype=torch.float32, device=dev)
        h_T = torch.empty((N, H), dtype=torch.float32, device=dev)
        need = any(ctx.needs_input_grad)
        saved = torch.empty((5, T * N, H), dtype=torch.float32, device=dev) if need else None
        c = Context.get(dev.index)
        ws, nbytes = _workspace(c, T, N, I, H, dev)
        c.check(c.lib.var_gru_seq_fwd(c.handle, current_stream_handle(), ptr(xs), ptr(hs), ptr(ms), ptr(wi), ptr(wh), ptr(bi),
                                      ptr(bh), T, N, I, H, ptr(out), ptr(h_T), ptr(saved), ptr(ws), nbytes),
                "var_gru_seq_fwd")
        if need:
            ctx.save_for_backward(xs, ms, wi, wh, saved)
        ctx.dims = (T, N, I, H)
        ctx.set_materialize_grads(False)
        ctx.mark_non_differentiable()
        return out, h_T

    @staticmethod
    @once_differentiable
    def backward(ctx, d_out, d_hT):
        xs, ms, wi, wh, saved = ctx.saved_tensors
        T, N, I, H = ctx.dims
        dev = xs.device
        if d_out is None:
            d_out = torch.zeros((T * N, H), dtype=torch.float32, device=dev)
        d_out = d_out.contiguous()
        if d_hT is not None:
            d_hT = d_hT.contiguous()
        d_x = torch.empty_like(xs)
        d_hxs = torch.empty((N, H), dtype=torch.float32, device=dev)
        d_wi, d_wh = torch.empty_like(wi), torch.empty_like(wh)
        d_bi = torch.empty(3 * H, dtype=torch.float32, device=dev)
        d_bh = torch.empty(3 * H, dtype=torch.float32, device=dev)
        c = Context.get(dev.index)
        ws, nbytes = _workspace(c, T, N, I, H, dev)
        c.check(c.lib.var_gru_seq_bwd(c.handle, current_stream_handle(), ptr(xs), ptr(ms), ptr(wi), ptr(wh), ptr(saved),
                                      ptr(d_out), ptr(d_hT), T, N, I, H, ptr(d_x), ptr(d_hxs), ptr(d_wi), ptr(d_wh), ptr(d_bi),
                                      ptr(d_bh), ptr(ws), nbytes),
                "var_gru_seq_bwd")
        return d_x, d_hxs, None, d_wi, d_wh, d_bi, d_bh


def masked_gru(x, hxs, masks, w_ih, w_hh, b_ih, b_hh):
    """x (T*N, I), hxs (N, H), masks (T*N, 1), the four nn.GRU parameters -> (out (T*N, H), h_T (N, H)); T = rows / N.
    Differentiable in x, hxs and the four parameters (var_gru_seq_bwd); masks carry no gradient.  H a multiple of 64 up to
    1024, I up to 1024, N up to 64.  Non-contiguous inputs are made contiguous."""
    return _MaskedGRU.apply(x, hxs, masks, w_ih, w_hh, b_ih, b_hh)


def _gru_parameters(gru):
    if not isinstance(gru, nn.GRU):
        raise VarHipError(f"forward_gru: an nn.GRU is expected, got {type(gru).__name__}")
    if gru.num_layers != 1 or gru.bidirectional or not gru.bias or getattr(gru, "proj_size", 0):
        raise VarHipError("forward_gru: an nn.GRU with one layer, one direction and biases (models/ppo/model.py:95)")
    return gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0


def forward_gru(gru, x, hxs, masks):
    """NNBase._forward_gru(x, hxs, masks) (models/ppo/model.py:116-171) for its nn.GRU: returns (x, hxs).  x.size(0) ==
    hxs.size(0) is the single-step branch (T = 1), anything else the (T*N, -1) sequence of a PPO minibatch."""
    return masked_gru(x, hxs, masks, *_gru_parameters(gru))


def bind_forward_gru(module):
    """Give a policy (anything with .base) or a base (anything with .gru) this op as its _forward_gru; returns the module.
    The reference's Policy, trained by var_amd.PPO, gets the op this way: PPO(bind_forward_gru(policy), ...)."""
    base = getattr(module, "base", module)
    if not hasattr(base, "gru"):
        raise VarHipError("bind_forward_gru: the module (or its .base) has no .gru")
    _gru_parameters(base.gru)
    base._forward_gru = types.MethodType(lambda self, x, hxs, masks: forward_gru(self.gru, x, hxs, masks), base)
    return module

"""CPU restatement of the acting forwards' bf16 mode (var_armnet_forward_ex / var_ithor_policy_forward_ex flags bit 0,
include/var_hip.h): tests/acting_layers_cpu.py's graph with `override`s that round x and w (convstack_bf16_cpu.bf16_round: nearest,
ties to even) in every imgCNN convolution node -- conv 1-8 of armNet_VAR, conv 1-6 of ai2thorNet_VAR -- and nothing else: the
bias, the pools, the occupancy convolutions, the MLP, the GRU cell and the head are acting_layers_cpu's own functions.  x_1 is the
float image formed in fp32 ((float)u8 / 255.f, or the float input) and then rounded, as the evaluation's oracle
(convstack_bf16_cpu.chain) forms it; tests/test_acting_bf16_host.py ties the two together.

The bound of a check is the project's convention (acting_layers_cpu, trunk_cpu): MARGIN = 4 times the distance of torch's fp32 CPU
evaluation of the SAME ROUNDED function on the same inputs from the float64 one, relative to the float64 array's largest magnitude;
never the kernel's output.  The operands are rounded before either evaluation, so a product is exact in both and what is left in
the distance is fp32 summation: the bounds are of the size of the fp32 forward's.  Where acting_layers_cpu.ORDER replaces torch's
fp32 by an emulation of the kernel's accumulation order, the same emulation runs on the rounded operands."""
import torch

from tests import acting_layers_cpu as al
from tests.acting_layers_cpu import MARGIN, ratio, rel  # noqa: F401
from tests.convstack_bf16_cpu import bf16_round

LAST = {"arm": "a8", "ipol": "a6"}
KIND = {"arm": 0, "ipol": 1}
PREFIX = "base.imgCNN."


def conv_nodes(model):
    """The imgCNN convolution nodes of the acting graph, in graph order (the occupancy stage is its own kind and stays fp32)."""
    return [k for k, node in al.graph(model).items() if node.kind == "conv"]


def _rounded(fn, first):
    if first:      # fn = conv1: the float image in fp32 first, then the rounding, then the layer in the weights' dtype
        return lambda image, w, b: al.conv3x3(bf16_round(al.image_input(image, torch.float32)).to(w.dtype), bf16_round(w), b)
    return lambda x, w, b: fn(bf16_round(x), bf16_round(w), b)


def overrides(model, skip=()):
    """{conv node: its function on rounded x and w}; `skip`: nodes left unrounded (the injected fault of a layer that forgot)."""
    G = al.graph(model)
    return {k: _rounded(G[k].fn, G[k].ins[0] == "image") for k in conv_nodes(model) if k not in skip}


def order_for(model, B):
    """acting_layers_cpu.order_for on rounded operands: {node: emulation of the kernel's order}, a convolution's after the rounding."""
    G = al.graph(model)
    return {k: (_rounded(fn, False) if G[k].kind == "conv" else fn) for k, fn in al.order_for(model, B).items()}


def chain(model, P, inputs, skip=()):
    """Every buffer of the rounded model from its inputs, in the dtype of the parameters P."""
    return al.chain(model, P, inputs, override=overrides(model, skip))


def check_layers(model, env, P, outputs, images=None, order=None, skip=(), log=None):
    """acting_layers_cpu.check_layers on the rounded graph: every buffer of `outputs` against float64 evaluated from the other
    buffers of env, {buffer: (span, error, distance, ratio)}; `order`: order_for(model, B); `skip`: as overrides."""
    G, ov, res = al.graph(model), overrides(model, skip), {}
    for out in outputs:
        sub = images is not None and out in al.MAPS[model] and G[out].kind != "pool"
        e = {k: (v[images] if sub else v) for k, v in env.items() if k != out}
        used = []
        ref = al.evaluate(G, out, e, P, torch.float64, override=ov, used=used)
        emu = {k: fn for k, fn in (order or {}).items() if k in [u for _kind, u in used]}
        dist = rel(al.evaluate(G, out, e, P, torch.float32, override={**ov, **emu}), ref)
        got = env[out][images] if sub else env[out]
        assert got.shape == ref.shape, (out, got.shape, ref.shape)
        err = rel(got, ref)
        span = "+".join(f"{kind}:{k}" for kind, k in reversed(used)) + (" (kernel order)" if emu else "")
        res[out] = (span, err, dist, ratio(err, dist))
        if log:
            log(f"{out:7s} {span:44s} err {err:.2e} dist {dist:.2e} ratio {res[out][3]:.3f}")
    return res


def end_to_end_distance(model, P, inputs):
    """({output: float64 value}, {output: distance}) of value, head and hout: torch's fp32 CPU evaluation of the WHOLE rounded graph
    from its inputs against the float64 one.  It contains what a map that lands on the other side of a bf16 rounding boundary in
    one of the two evaluations does to everything above it."""
    ref = chain(model, {k: v.double() for k, v in P.items()}, inputs)
    f32 = chain(model, {k: v.float() for k, v in P.items()}, inputs)
    return {k: ref[k] for k in al.OUTPUTS}, {k: rel(f32[k], ref[k]) for k in al.OUTPUTS}


def policy_tensors(kind, seed, n_act):
    """convstack_cpu.policy_params as fp32 tensors by state_dict key."""
    from tests import convstack_cpu as cc
    return {k: torch.from_numpy(v).float() for k, v in cc.policy_params(kind, seed, n_act).items()}

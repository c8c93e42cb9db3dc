"""Host checks of the acting forwards' bf16 mode (var_armnet_forward_ex / var_ithor_policy_forward_ex flags bit 0;
policy.set_acting_precision): the exported entries, the CPU restatement tests/acting_bf16_cpu.py against the EVALUATION's oracle
(convstack_bf16_cpu.chain: acting and evaluation round at the same points), that the rounding is visible to the layer checks of
tests/test_gpu_acting_bf16.py (a convolution that forgot to round exceeds its layer's bound), and the Python setting's validation."""
import ctypes

import pytest
import torch

from tests import acting_bf16_cpu as ab
from tests import acting_layers_cpu as al
from tests import convstack_bf16_cpu as cb
from tests import convstack_cpu as cc
from tests import trunk_cpu as tc

MODELS = ("arm", "ipol")
N_ACT = {"arm": 2, "ipol": 8}


def test_the_library_exports_the_ex_entries():
    import var_amd
    from var_amd import _lib
    lib = ctypes.CDLL(var_amd.library_path())
    for name in ("var_armnet_forward_ex", "var_ithor_policy_forward_ex"):
        assert name in _lib.EXPORTED_SYMBOLS, name
        assert getattr(lib, name) is not None
        old = name[:-3]
        assert len(_lib._SIGNATURES[name][1]) == len(_lib._SIGNATURES[old][1]) + 1 and _lib._SIGNATURES[name][1][-1] is ctypes.c_int


@pytest.mark.parametrize("model", MODELS)
def test_the_rounded_acting_graph_is_the_evaluations_oracle(model):
    kind, B, seed = ab.KIND[model], 2, 23
    P = ab.policy_tensors(kind, seed, N_ACT[model])
    stack = {k[len(ab.PREFIX):]: v.numpy() for k, v in P.items() if k.startswith(ab.PREFIX)}
    d = cc.convstack_data(kind, B, seed)
    want = cb.chain(kind, stack, d, torch.float64)["feat"]
    G = al.graph(model)
    env = {"image": torch.from_numpy(d["image"])}
    got = al.evaluate(G, ab.LAST[model], env, {k: v.double() for k, v in P.items()}, torch.float64, override=ab.overrides(model))
    assert got.shape == want.shape == (B, 1152) and got.dtype == torch.float64
    assert float(want.abs().max()) > 0 and bool((want == 0).any())
    assert float((got - want).abs().max()) <= 1e-12 * float(want.abs().max())
    # a float image (the bytes already divided in fp32) gives the same function
    envf = {"image": torch.from_numpy(cc.as_float_image(d["image"]))}
    gotf = al.evaluate(G, ab.LAST[model], envf, {k: v.double() for k, v in P.items()}, torch.float64, override=ab.overrides(model))
    assert torch.equal(gotf, got)
    # every imgCNN convolution is overridden and nothing else
    assert ab.conv_nodes(model) == [k for k in al.MAPS[model] if k.startswith("a")]
    assert sorted(ab.overrides(model)) == sorted(ab.conv_nodes(model)) and "occf" not in ab.overrides(model)


@pytest.mark.parametrize("model", MODELS)
def test_a_convolution_that_forgot_to_round_exceeds_its_layers_bound(model):
    kind, B = ab.KIND[model], 2
    P = ab.policy_tensors(kind, 29, N_ACT[model])
    inputs = al.random_inputs(model, B, 29)
    G = al.graph(model)
    with torch.no_grad():
        clean = ab.chain(model, P, inputs)                           # fp32, every imgCNN convolution rounded
        plain = al.chain(model, P, inputs)                           # fp32, unrounded
        keep = [k for k in al.survivors(model, B) if k in al.MAPS[model] and k != "occf"]
        assert keep == (["a1", "p1", "a3", "p2", "a5", "p3", "a7", "a8"] if model == "arm" else ["a1", "p1", "p2", "p3", "p4", "a6"])
        for k in keep:                                                # the override is not a no-op, layer by layer
            assert not torch.equal(clean[k], plain[k]), k
            assert ab.rel(clean[k], plain[k]) < 0.05, k               # (and a bf16 product's worth, not another function)
        assert torch.equal(clean["occf"], plain["occf"]) if model == "ipol" else True
        env = dict(inputs, **{k: clean[k] for k in al.survivors(model, B)})
        res = ab.check_layers(model, env, P, keep)
        assert all(r[3] <= 1 for r in res.values()), res              # the clean buffers pass their own checks
        for k in keep:
            conv = k if G[k].kind == "conv" else G[k].ins[0]
            e = {q: v for q, v in env.items() if q != k}
            bad = al.evaluate(G, k, e, P, torch.float32, override=ab.overrides(model, skip=(conv,)))
            r = ab.check_layers(model, dict(env, **{k: bad}), P, [k])[k]
            print(f"{model} {k}: {conv} left unrounded: err {r[1]:.2e} dist {r[2]:.2e} ratio {r[3]:.1f}")
            assert r[3] > 1, (k, r)
            # and the fp32 forward's own checker (unrounded float64) refuses the rounded buffer likewise
            assert al.check_layers(model, env, P, [k])[k][3] > 1, k


def test_the_acting_precision_setting_is_validated_without_a_device():
    import var_amd
    for kind in (0, 1):
        pol = tc.drop_in_policy(kind, 0)
        assert pol.acting_precision == "fp32"
        for bad in ("fp16", "BF16", None, 1):
            with pytest.raises(var_amd.VarHipError, match="precision"):
                pol.set_acting_precision(bad)
        assert pol.acting_precision == "fp32"
        assert pol.set_acting_precision("bf16") is pol and pol.acting_precision == "bf16"
        assert pol.set_acting_precision("fp32").acting_precision == "fp32"
        with pytest.raises(var_amd.VarHipError, match="precision"):
            pol.capture(8, precision="fp16")                          # (refused before anything asks for a device)

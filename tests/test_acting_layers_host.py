"""The checker of tests/test_gpu_acting_layers.py, pinned on the CPU (tests/acting_layers_cpu.py): chained in float64 its layer
functions ARE the two actor-critics (oracle.torch_oracle.ArmNetCPU in .double(), tests/ithor_policy_cpu.forward in float64, to
1e-12); with torch's fp32 kernels standing in for the device every single-layer check passes on every route; and each fault a
kernel of this kind can have -- injected into ONE buffer, everything upstream intact -- fails the check of that buffer.  For the
record (printed, and tabulated in DESIGN section 7): how far each fault moves value / head / rnn_hxs_out, which is all the
output-only tests see at atol 2e-5.  No GPU needed."""
import functools
import types

import pytest
import torch

from oracle.torch_oracle import armnet_seeded
from tests import acting_layers_cpu as al
from tests.ithor_policy_cpu import forward as ithor_forward

B = 3
OLD_ATOL = 2e-5                    # tests/test_gpu_armnet.py, tests/test_gpu_ithor_policy.py: the outputs against torch fp32
MODELS = ("arm", "ipol")


class Discrete:
    n = 8


@functools.lru_cache(maxsize=None)
def params(model):
    if model == "arm":
        sd = armnet_seeded(453).state_dict()
    else:
        import var_amd
        torch.manual_seed(977)
        sd = var_amd.IthorNetPolicy(None, Discrete(), config=types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3),
                                    base='ai2thor_VAR', base_kwargs={'recurrent': True, 'recurrentInputSize': 128,
                                                                     'recurrentSize': 1024, 'actionHiddenSize': 128}).state_dict()
    return {k: v.detach().clone().float() for k, v in sd.items()}


@functools.lru_cache(maxsize=None)
def clean(model, seed=21):
    """(inputs, fp32 chain) of one call: torch's fp32 CPU kernels standing in for the device."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    inputs = al.random_inputs(model, B, seed, u8=seed % 2 == 1)
    with torch.no_grad():
        return inputs, al.chain(model, params(model), inputs)


@pytest.mark.parametrize("model", MODELS)
def test_float64_chain_is_the_model(model):
    P64 = {k: v.double() for k, v in params(model).items()}
    inputs = clean(model)[0]
    img = al.image_input(inputs["image"], torch.float64)
    with torch.no_grad():
        b = al.chain(model, P64, inputs)
        if model == "arm":
            m = armnet_seeded(453).double()
            obs = {"image": img, "image_feat": inputs["image_feat"].double(), "robot_pose": inputs["robot_pose"].double(),
                   "goal_sound_feat": inputs["goal"].double()}
            value, head, _lp, hout, feats = m.act_deterministic(obs, inputs["hxs"].double(), inputs["masks"].double())
        else:
            occ = inputs["occupancy"].double() / 255
            value, feats, head, hout = ithor_forward(P64, img, occ, inputs["image_feat"], inputs["goal"], inputs["hxs"], inputs["masks"],
                                                     dtype=torch.float64)
    for k, want in (("value", value), ("feats", feats), ("head", head), ("hout", hout)):
        assert b[k].dtype == torch.float64 and b[k].shape == want.shape
        assert float((b[k] - want).abs().max()) <= 1e-12, k
    assert not (inputs["masks"] == 1).all() and not (inputs["masks"] == 0).all()


@pytest.mark.parametrize("rows", [al.CHAIN_ROWS, al.CHAIN_ROWS + 1, al.BAND_MAX_B + 1])
@pytest.mark.parametrize("model", MODELS)
def test_torch_fp32_passes_every_layer_on_every_route(model, rows):
    inputs, b = clean(model)
    keep = al.survivors(model, rows)
    env = dict(inputs, **{k: b[k] for k in keep})
    with torch.no_grad():
        res = al.check_layers(model, env, params(model), keep, log=lambda s: print(f"{model} route of B={rows}: {s}"))
    assert list(res) == keep and set(al.OUTPUTS) <= set(keep)
    assert len(keep) == {"arm": (32, 23, 26), "ipol": (32, 23, 27)}[model][(rows > al.CHAIN_ROWS) + (rows > al.BAND_MAX_B)]
    bad = {k: r for k, r in res.items() if not r[3] <= 1}
    assert not bad, bad
    exact = [k for k, r in res.items() if r[2] == 0]
    assert exact == [k for k in keep if k == "h0" or (k.startswith("p") and rows > al.BAND_MAX_B)], exact      # routing: bound 0


@pytest.mark.parametrize("model", MODELS)
def test_every_fault_fails_the_check_of_its_buffer(model):
    inputs, b = clean(model)
    other = clean(model, seed=22)[1]
    P = params(model)
    keep = al.survivors(model, al.CHAIN_ROWS)
    env = dict(inputs, **{k: b[k] for k in keep})
    G = al.graph(model)
    with torch.no_grad():
        table = al.faults(model, env, P, other)
        kinds = {f for f, _k, _y in table}
        assert len(kinds) == 10, kinds
        missed = []
        for fault, k, y in table:
            assert y.shape == env[k].shape and not torch.equal(y, env[k]), (fault, k)
            span, err, dist, q = al.check_layers(model, dict(env, **{k: y}), P, [k])[k]
            # what the output-only tests see: the rest of the forward from the faulty buffer, against the clean outputs
            seen = dict(inputs, **{k: y})
            moved = max(al.rel(y if o == k else al.evaluate(G, o, seen, P, torch.float32), b[o], 1.0) for o in al.OUTPUTS)      # (NaN: inf)
            old = "passes" if moved <= OLD_ATOL else "fails"
            print(f"{model:4s} {fault:40s} {k:6s} layer check: {q:10.3g} x its bound; outputs move {moved:.1e}: {old} at atol {OLD_ATOL}")
            if not q > 1:
                missed.append((fault, k, err, dist, q))
    assert not missed, missed


def test_the_two_order_yardsticks_still_catch_a_fault():
    """acting_layers_cpu.ORDER replaces torch's distance by the kernel order's for Kuka's conv 6 on the gather-GEMM route and
    for its value layer on the chain: the clean buffers pass those checks too, a dropped tap / the neighbouring row does not."""
    inputs, b = clean("arm")
    P, G = params("arm"), al.graph("arm")
    assert set(al.order_for("arm", al.BAND_MAX_B + 1)) == {"a6"} and set(al.order_for("arm", al.CHAIN_ROWS)) == {"value"}
    assert not al.order_for("arm", al.BAND_MAX_B) and not al.order_for("ipol", al.BAND_MAX_B + 1) and not al.order_for("ipol", 1)
    with torch.no_grad():
        w = P["base.imgCNN.12.weight"].clone()
        w[:, :16, 2, 2] = 0
        c1 = b["c1"].roll(1, 0)
        for rows, k, faulty in ((al.BAND_MAX_B + 1, "a6", al.conv3x3(b["a5"], w, P["base.imgCNN.12.bias"])),
                                (al.CHAIN_ROWS, "value", G["value"].fn(c1, P["base.critic_linear.weight"], P["base.critic_linear.bias"]))):
            env = dict(inputs, **{n: b[n] for n in al.survivors("arm", rows)})
            order = al.order_for("arm", rows)
            span, _err, dist, q = al.check_layers("arm", env, P, [k], order=order)[k]
            assert span.endswith("(kernel order)") and dist > 0 and q <= 1, (k, span, dist, q)
            q = al.check_layers("arm", dict(env, **{k: faulty}), P, [k], order=order)[k][3]
            assert q > 1e3, (k, q)

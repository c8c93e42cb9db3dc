"""Host-side checks of the actor-critics' convolution stacks (csrc/convstack.hip, var_amd.conv_stack_eval): the float64 checker
against the fixtures made from the reference, the gate- and choice-taking restatement against plain autograd, the published
parameter order and offsets, the exported symbols and the refusals that need no GPU.  No GPU."""
import os
import types

import numpy as np
import pytest
import torch

import var_amd
from tests import convstack_cpu as cc
from tests import trunk_cpu as tc
from var_amd import convstack as vc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def stack_module(kind):
    """The drop-in policies' module of a kind (the reference's layers under the reference's names)."""
    base = tc.drop_in_policy(1 if kind else 0, 0).base
    return base.occupancyCNNMLP if kind == 2 else base.imgCNN


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_checker_reproduces_reference_fixture(kind):
    g = cc.load_fixture(GOLDEN, kind)
    assert g["image"].dtype == np.uint8 and g["image"].shape == (cc.FIXTURE_B,) + cc.STACKS[kind][0]
    P, d = cc.fixture_inputs(kind, g)
    got = cc.evaluate(kind, P, d, torch.float64)
    dist = cc.fixture_distances(kind, {k: v for k, v in got.items() if k == "feat" or k.startswith("d.")}, g)
    worst = max(dist, key=dist.get)
    print(f"kind {kind}: {len(dist)} arrays, worst {worst} {dist[worst]:.2e}")
    n = len(cc.layer_names(kind))
    assert len(dist) == 1 + n + 3 * n                      # feat, the bias gradients, rows16 / rowsum / colsum per weight gradient
    assert all(v <= 1e-6 for v in dist.values()), {k: v for k, v in dist.items() if v > 1e-6}


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_gated_form_is_plain_autograd_at_its_own_gates_and_choices(kind):
    P, d = cc.convstack_params(kind, 11), cc.convstack_data(kind, 2, 11)
    a = cc.evaluate(kind, P, d, torch.float64)
    b = cc.evaluate(kind, P, d, torch.float64, gates=cc.gates_of(a, kind), choices=cc.choices_of(a, kind))
    assert set(a) == set(b)
    for k in a:
        assert cc.rel(b[k], a[k]) <= 1e-12, k
    # foreign gates and choices change the function: the arguments are really used
    other = cc.evaluate(kind, cc.convstack_params(kind, 12), d, torch.float64)
    c = cc.evaluate(kind, P, d, torch.float64, gates=cc.gates_of(other, kind), choices=cc.choices_of(other, kind))
    assert cc.rel(c["feat"], a["feat"]) > 1e-3
    assert cc.flipped_units(kind, a, a, {"act." + n: 1e-7 for n in cc.layer_names(kind)}) == (0, 0.0)
    assert cc.flipped_units(kind, other, a, {"act." + n: 1e-7 for n in cc.layer_names(kind)})[0] > cc.MAX_FLIPS


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_published_parameter_order_and_offsets(kind):
    lib = var_amd.load_library()
    mod = stack_module(kind)
    assert vc.stack_kind(mod) == kind
    names = vc.stack_param_names(kind)
    assert names == cc.param_names(kind)
    sd = mod.state_dict()
    convs = [k for k, v in sd.items() if v.dim() in (1, 4)][:len(names)] if kind == 2 else list(sd)
    assert convs == names                                                        # state_dict order
    assert lib.var_convstack_n_params(kind) == len(names)
    params = vc.stack_parameters(mod)
    end = 0
    for i, (name, p) in enumerate(zip(names, params)):
        cin, cout = cc.STACKS[kind][1][i // 2][:2]
        assert tuple(p.shape) == ((cout, cin, 3, 3) if i % 2 == 0 else (cout,))
        assert p.data_ptr() == sd[name].data_ptr()
        assert lib.var_convstack_param_floats(kind, i) == p.numel()
        assert lib.var_convstack_grad_offset(kind, i) == end                    # the flat gradient buffer: dense, in order
        end += p.numel()
    assert lib.var_convstack_grad_offset(kind, len(names)) == end
    for B in (1, 3, 15, 1024):
        m, end = vc.saved_map(kind, B), 0
        assert list(m) == list(cc.layer_names(kind))
        for name, shape in cc.map_shapes(kind, B).items():
            assert m[name] == (end, shape) and end % 4 == 0
            end += int(np.prod(shape))
        assert lib.var_convstack_saved_offset(kind, B, len(m)) == lib.var_convstack_saved_floats(kind, B) == end
        assert shape[1] * shape[2] * shape[3] == cc.feat_width(kind)
        assert lib.var_convstack_workspace_bytes(kind, B) > 0
    for bad in ((kind, 0), (kind, 1025), (3, 4), (-1, 4)):
        assert lib.var_convstack_workspace_bytes(*bad) == -1 and lib.var_convstack_saved_floats(*bad) == -1
        assert lib.var_convstack_saved_offset(*bad, 0) == -1
    assert lib.var_convstack_n_params(3) == -1 and lib.var_convstack_param_floats(kind, len(names)) == -1
    assert lib.var_convstack_grad_offset(kind, len(names) + 1) == -1 and lib.var_convstack_saved_offset(kind, 4, len(names) // 2 + 1) == -1


def test_library_exports_the_convstack_symbols():
    from var_amd._lib import EXPORTED_SYMBOLS
    lib = var_amd.load_library()
    for name in ("var_convstack_n_params", "var_convstack_param_floats", "var_convstack_grad_offset", "var_convstack_saved_floats",
                 "var_convstack_saved_offset", "var_convstack_workspace_bytes", "var_convstack_fwd", "var_convstack_bwd"):
        assert name in EXPORTED_SYMBOLS
        getattr(lib, name)
    assert callable(var_amd.conv_stack_eval) and callable(var_amd.bind_convs)


def test_cpu_tensors_and_foreign_modules_are_refused():
    import torch.nn as nn
    mod = stack_module(0)
    with pytest.raises(var_amd.VarHipError, match="CUDA"):
        var_amd.conv_stack_eval(mod, torch.zeros(2, 3, 96, 96))
    # buildCNN's other branch (7 x 7 filter, 120 x 160 images) is out of scope
    other = nn.Sequential(nn.Conv2d(3, 64, 7, stride=2, padding=1), nn.ReLU(), nn.Conv2d(64, 64, 3, stride=1, padding=1), nn.ReLU(),
                          nn.MaxPool2d(2, stride=2), nn.Flatten())
    with pytest.raises(var_amd.VarHipError, match="7 x 7"):
        var_amd.conv_stack_eval(other, torch.zeros(1, 3, 120, 160))
    with pytest.raises(var_amd.VarHipError):
        var_amd.conv_stack_eval(nn.Linear(2, 2), torch.zeros(1, 3, 96, 96))
    with pytest.raises(var_amd.VarHipError):
        var_amd.bind_convs(nn.Linear(2, 2))
    pol = tc.drop_in_policy(0, 0)
    pol.base.imgCNN = tc.standin_modules(0)[0]
    with pytest.raises(var_amd.VarHipError):
        var_amd.bind_convs(pol)
    assert var_amd.bind_convs(tc.drop_in_policy(1, 0)).base.forward.__func__ is vc._convs_forward
    other = types.SimpleNamespace(base=torch.nn.Module())
    with pytest.raises(var_amd.VarHipError):
        var_amd.bind_convs(other)

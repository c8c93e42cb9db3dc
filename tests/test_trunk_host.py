"""Host-side checks of the PPO update's MLP trunk (csrc/trunk.hip, var_amd.trunk_eval): the float64 checker against the fixtures
made from the reference, the gated form, the published parameter order, the exported symbols, the refusal of CPU tensors, and an
fp32 emulation of the kernels' summation order against the bounds the GPU tests use.  No GPU."""
import os
import types

import numpy as np
import pytest
import torch

import var_amd
from tests import trunk_cpu as tc
from var_amd import trunk as vt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (kind, T, N) of tests/test_gpu_trunk.py
CASES = [(k, T, N) for k in (0, 1) for T, N in ((1, 1), (3, 2), (2, 17), (7, 5))] + [(0, 33, 4), (1, 1, 5)]


make_policy = tc.drop_in_policy


@pytest.mark.parametrize("kind", [0, 1])
def test_checker_reproduces_reference_fixture(kind):
    g = tc.load_fixture(GOLDEN, kind)
    P, d = tc.fixture_inputs(kind, g)
    got = tc.evaluate(kind, P, d, torch.float64, variants=("no_d_hT",))["no_d_hT"]
    dist = tc.fixture_distances(kind, got, g)
    worst = max(dist, key=dist.get)
    print(f"kind {kind}: {len(dist)} arrays, worst {worst} {dist[worst]:.2e}")
    assert len(dist) == 3 + 2 + kind + len(tc.param_names(kind)) + 2 * (2 + len(tc.layers(kind)))
    assert all(v <= 1e-6 for v in dist.values()), {k: v for k, v in dist.items() if v > 1e-6}


@pytest.mark.parametrize("kind", [0, 1])
def test_gated_form_is_the_relu_form_at_its_own_gates(kind):
    P, d = tc.trunk_inputs(kind, 3, 2, 11)
    a = tc.evaluate(kind, P, d, torch.float64, variants=tuple(tc.VARIANTS))
    b = tc.evaluate(kind, P, d, torch.float64, gates=tc.gates_of(a["all"], kind), variants=tuple(tc.VARIANTS))
    for v in tc.VARIANTS:
        for k in a[v]:
            assert np.array_equal(a[v][k], b[v][k]), (v, k)


@pytest.mark.parametrize("kind", [0, 1])
def test_published_parameter_order(kind):
    lib = var_amd.load_library()
    pol = make_policy(kind, 0)
    names = vt.trunk_param_names(kind)
    assert names == tc.param_names(kind)
    trunk = set(names)
    assert [k for k in pol.base.state_dict() if k in trunk] == names            # state_dict order
    assert lib.var_trunk_n_params(kind) == len(names) == 4 + 2 * lib.var_trunk_n_layers(kind)
    params = vt.trunk_parameters(pol.base)
    sd, end = pol.base.state_dict(), 0
    for i, (name, p) in enumerate(zip(names, params)):
        assert p.data_ptr() == sd[name].data_ptr()
        assert lib.var_trunk_param_floats(kind, i) == p.numel()
        assert lib.var_trunk_grad_offset(kind, i) >= end                        # the flat gradient buffer: no overlap
        end = lib.var_trunk_grad_offset(kind, i) + p.numel()
    assert lib.var_trunk_grad_offset(kind, len(names)) >= end
    # the saved activations: one slice per layer, then the GRU's
    m, end = vt.saved_map(kind, 7, 5), 0
    assert list(m)[:-2] == [name for name, *_ in tc.layers(kind)]
    for (off, rows, cols), (_n, _i, o, _s, _r) in zip(m.values(), tc.layers(kind)):
        assert off >= end and rows == 35 and cols == o
        end = off + rows * cols
    assert m["gru"][0] >= end and m["gru.saved"][0] >= m["gru"][0] + 35 * tc.hidden(kind)
    assert lib.var_trunk_saved_floats(kind, 7, 5) >= m["gru.saved"][0] + 5 * 35 * tc.hidden(kind)
    assert lib.var_trunk_workspace_bytes(kind, 7, 5) > 0
    for bad in ((kind, 0, 5), (kind, 7, 0), (kind, 7, 65), (2, 7, 5), (kind, 16385, 1)):
        assert lib.var_trunk_workspace_bytes(*bad) == -1 and lib.var_trunk_saved_floats(*bad) == -1


def test_library_exports_the_trunk_symbols():
    from var_amd._lib import EXPORTED_SYMBOLS
    lib = var_amd.load_library()
    for name in ("var_trunk_n_layers", "var_trunk_n_params", "var_trunk_param_floats", "var_trunk_grad_offset",
                 "var_trunk_saved_offset", "var_trunk_saved_floats", "var_trunk_workspace_bytes", "var_trunk_fwd", "var_trunk_bwd"):
        assert name in EXPORTED_SYMBOLS
        getattr(lib, name)
    assert callable(var_amd.trunk_eval) and callable(var_amd.bind_trunk)


@pytest.mark.parametrize("kind", [0, 1])
def test_cpu_tensors_are_refused(kind):
    pol = make_policy(kind, 0)
    _P, d = tc.trunk_inputs(kind, 2, 2, 5)
    t = {k: torch.from_numpy(v) for k, v in d.items()}
    with pytest.raises(var_amd.VarHipError, match="CUDA"):
        var_amd.trunk_eval(pol.base, t["feat"], t["motor_in"], t["sound_in"], t["hxs"], t["masks"], occ=t.get("occ"))
    with pytest.raises(var_amd.VarHipError):
        var_amd.bind_trunk(torch.nn.Linear(2, 2))
    other = types.SimpleNamespace(base=torch.nn.Module())
    other.base.gru = torch.nn.GRU(128, 256)
    with pytest.raises(var_amd.VarHipError):
        var_amd.bind_trunk(other)


@pytest.mark.parametrize("kind,T,N", CASES)
def test_emulated_summation_order_within_half_the_bound(kind, T, N):
    seed = tc.find_seed(kind, T, N, 100 * (kind + 1) + T + N)
    P, d = tc.trunk_inputs(kind, T, N, seed)
    variants = tuple(tc.VARIANTS)
    em = tc.emulate(kind, P, d, variants)
    gates = tc.gates_of(em["all"], kind)
    ref_fwd = tc.evaluate(kind, P, d, torch.float64)["all"]
    ref = tc.evaluate(kind, P, d, torch.float64, gates=gates, variants=variants)
    dist = tc.trunk_distance(kind, T, N)
    flips, ratio = tc.flipped_gates(kind, gates, ref_fwd, dist["all"])
    assert flips <= tc.MAX_FLIPS and ratio <= 1.0, (flips, ratio)
    worst = (0.0, None)
    for v in variants:
        for k in tc.compared_keys(ref[v]):
            r = ref_fwd if k.startswith(("value", "actor_features", "h_T", "act.")) else ref[v]
            bound = tc.MARGIN * dist[v][k]
            err = tc.rel(em[v][k], r[k])
            worst = max(worst, (err / bound if bound else (0.0 if err == 0 else np.inf), (v, k, err, bound)))
    print(f"kind {kind} T {T} N {N} seed {seed}: flipped gates {flips}, worst error / bound {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 0.5, worst

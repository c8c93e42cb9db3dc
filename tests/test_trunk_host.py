"""Host-side checks of the PPO update's MLP trunk (csrc/trunk.hip, var_amd.trunk_eval): the float64 checker against the fixtures
made from the reference, the gated form, the published parameter order, the exported symbols, the refusal of CPU tensors, and an
fp32 emulation of the kernels' summation order against the bounds the GPU tests use; and, with torch's fp32 CPU evaluation standing
in for the device, the faults that the row counts of trunk_cpu.THRESHOLD_SHAPES are there to catch, injected one at a time: each is
rejected by that shape's bound and could not have shown at 132 rows, the most the GPU tests ran before.  No GPU."""
import os
import types

import numpy as np
import pytest
import torch

import var_amd
from tests import trunk_cpu as tc
from var_amd import trunk as vt

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# (kind, T, N) of tests/test_gpu_trunk.py's small cases (the emulation below is a Python loop over k: minutes at 1000 rows)
CASES = [(k, T, N) for k in (0, 1) for T, N in ((1, 1), (3, 2), (2, 17), (7, 5))] + [(0, 33, 4), (1, 1, 5)]
CASES.append((0, 6, 43))                     # 258 rows: the smallest with a second pass in column_sums


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
    dist = tc.case_distance(kind, T, N)
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


# ---- the shapes at which the kernels change their tiling: what they are for, and that their bounds would notice -------------------
def test_threshold_shapes_sit_where_the_tile_rule_switches():
    """tc.tile_rows restates product_job's rule; the first row count with 32-row tiles, per output width J."""
    first = {J: next(I for I in range(1, 20000) if tc.tile_rows(I, J) == 32) for J in (1152, 1024, 512, 288, 256, 128, 64, 5)}
    assert first == {1152: 225, 1024: 225, 512: 481, 288: 897, 256: 993, 128: 2017, 64: 4065, 5: 8161}
    rows = sorted(T * N for T, N in tc.THRESHOLD_SHAPES)
    assert rows == [224, 225, 258, 481, 513, 992, 1000] and all(N <= 64 for _T, N in tc.THRESHOLD_SHAPES)
    assert [len(tc.column_passes(r)) for r in rows] == [1, 1, 2, 2, 3, 4, 4] and tc.column_passes(258)[-1] == (256, 2)
    assert tc.column_passes(513)[-1] == (512, 1)
    for kind in (0, 1):                                            # up to 132 rows no product with rows = T * N took the 32-row tile
        for T, N in tc.SMALL_SHAPES[kind]:
            assert all(tc.tile_rows(T * N, J) == 16 for _n, i, o, _s, _r in tc.layers(kind) for J in (i, o, 1152, tc.hidden(kind)))
            assert len(tc.column_passes(T * N)) == 1
    assert max(T * N for T, N in tc.SMALL_SHAPES[0]) == 132 == tc.LARGEST_SMALL[0] * tc.LARGEST_SMALL[1]


def _stand_in(kind, T, N):
    """torch's fp32 CPU evaluation standing in for the device at a GPU case's own inputs: (fp32 results, fp32 pre-activation
    gradients, float64 results, bounds of the 'all' variant)."""
    seed = tc.find_seed(kind, T, N, 100 * (kind + 1) + T + N)
    P, d = tc.trunk_inputs(kind, T, N, seed)
    t32 = tc.evaluate(kind, P, d, torch.float32)["all"]
    ref = tc.evaluate(kind, P, d, torch.float64)["all"]            # (find_seed: both have the same gates)
    n = tc.draws(T, N)
    dist = tc.trunk_distance(kind, T, N, n, ("all",))["all"] if (T, N) in tc.THRESHOLD_SHAPES else tc.trunk_distance(kind, T, N)["all"]
    return t32, tc.pre_activation_gradients(kind, P, d, torch.float32), ref, {k: tc.MARGIN * v for k, v in dist.items()}


@pytest.mark.parametrize("fault", ["first_pass_only", "last_pass_twice"])
def test_bias_gradient_faults_are_rejected_at_258_rows(fault):
    """column_sums with a second pass gone wrong, in every layer's bias gradient, against the (6, 43) case's bounds; at 132 rows,
    the largest size run before, there is one pass and the fault changes no bit."""
    kind = 0
    _t32, G, ref, bound = _stand_in(kind, 6, 43)
    worst_ok, least = 0.0, np.inf
    for name, *_ in tc.layers(kind):
        k = "d." + name + ".bias"
        worst_ok = max(worst_ok, tc.rel(tc.faulty_column_sums(G[name]), ref[k]) / bound[k])
        least = min(least, tc.rel(tc.faulty_column_sums(G[name], fault), ref[k]) / bound[k])
    print(f"{fault} at 258 rows: the sound sum is at most {worst_ok:.3f} of its bound, the fault at least {least:.3g} x")
    assert worst_ok <= 1.0 and least > 1.0, (worst_ok, least)
    _t32, G, _ref, _bound = _stand_in(kind, *tc.LARGEST_SMALL)
    for name, *_ in tc.layers(kind):
        assert np.array_equal(tc.faulty_column_sums(G[name], fault), tc.faulty_column_sums(G[name])), name


@pytest.mark.parametrize("fault", ["last_row_zero", "last_row_repeats", "halves_exchanged"])
def test_ragged_32_row_tile_faults_are_rejected_at_225_rows(fault):
    """d_feat at (15, 15) is 225 x 1152 on 32-row tiles, the last holding one row; at 132 rows it was on 16-row tiles, whose ragged
    edge the small cases did run (132 = 8 * 16 + 4), so product_tile<2>'s clamp and guards ran for no row there."""
    kind = 0
    t32, _G, ref, bound = _stand_in(kind, 15, 15)
    assert tc.tile_rows(225, 1152) == 32 and 225 % 32 == 1 and tc.tile_rows(132, 1152) == 16
    ok = tc.rel(t32["d_feat"], ref["d_feat"]) / bound["d_feat"]
    bad = tc.rel(tc.faulty_tile_rows(t32["d_feat"], fault), ref["d_feat"]) / bound["d_feat"]
    print(f"{fault} in d_feat at 225 rows: sound {ok:.3f} of the bound, the fault {bad:.3g} x")
    assert ok <= 1.0 < bad, (ok, bad)

"""Host-side checks of the support code of the convolution stacks' large-batch tests (tests/convstack_large_cpu.py): the Python
restatement of csrc/convstack.hip's split and workspace arithmetic against the library and the recorded split counts, the
repeated-image reduction against the full float64 evaluation, the new bound against injected faults, and the kernels' own order
of additions emulated in fp32.  No GPU."""
import numpy as np
import pytest
import torch

import var_amd
from tests import convstack_bf16_cpu as cb
from tests import convstack_cpu as cc
from tests import convstack_large_cpu as cl


# ---- 1: the restatement -----------------------------------------------------------------------------------------------------------------
def test_split_counts_are_the_recorded_ones_and_the_first_cap_sizes_the_table_s():
    # DESIGN.md's per-kernel table (rocprofv3, kind 0 at B = 400)
    assert [cl.wgrad_split(0, l, 400) for l in range(8)] == [1020, 128, 128, 128, 103, 57, 29, 23]
    p = cl.wgrad_plan(0, 7, 400)
    assert (p["splits"], p["per"], p["last"]) == (23, 5, 3)
    caps = {k: [cl.wgrad_plan(k, l, 1)["cap"] for l in range(len(cc.layer_names(k)))] for k in (0, 1, 2)}
    first = {k: [cl.first_cap_batch(k, l) for l in range(len(cc.layer_names(k)))] for k in (0, 1, 2)}
    assert caps == {0: [1024, 128, 128, 128, 103, 57, 29, 29], 1: [1024, 128, 128, 128, 103, 57], 2: [128, 128]}
    assert first == {0: [15, 2, 8, 8, 23, 13, 148, 409], 1: [15, 2, 8, 29, 92, 808], 2: [1017, 1017]}
    for k in (0, 1, 2):                                             # a cap that holds keeps holding, and none is exceeded
        for l in range(len(cc.layer_names(k))):
            held = [cl.cap_holds(k, l, B) for B in range(1, cl.MAX_BATCH + 1)]
            assert held == sorted(held)
            assert all(1 <= cl.wgrad_split(k, l, B) <= caps[k][l] for B in range(1, cl.MAX_BATCH + 1))
    # chain lengths of the issue: conv 2's splits, a bias thread on a 96 x 96 map
    assert [cl.wgrad_plan(0, 1, B)["per"] for B in (25, 400, 1024)] == [57, 900, 2304]
    assert [cl.chan_sum_chain(0, 0, B) for B in (400, 1024)] == [450, 1152]


def test_the_case_table_comes_from_the_restatement():
    cases = cl.cases()
    for line in (row for c in cases for row in cl.describe(*c)):
        print(line)
    sizes = {k: sorted({B for kk, B, _l in cases if kk == k}) for k in (0, 1, 2)}
    assert sizes == {0: [147, 148, 200, 400, 408, 409, 1024], 1: [28, 29, 91, 92, 200, 807, 808, 1024], 2: [200, 1023, 1024]}
    single = {(k, B): layers for k, B, layers in cases if len(layers) == 1}
    assert single == {(0, 147): ("15",), (0, 148): ("15",), (0, 408): ("17",), (0, 409): ("17",), (1, 28): ("8",), (1, 29): ("8",),
                      (1, 91): ("11",), (1, 92): ("11",), (1, 807): ("14",), (1, 808): ("14",)}
    for k, B, layers in cases:
        if len(layers) > 1:
            assert layers == cc.layer_names(k)
    assert cl.wgrad_plan(2, 0, 1023)["last"] == 7 and cl.wgrad_plan(2, 0, 1023)["splits"] == 128      # the ragged 128th slab
    # the layers the gather-GEMM serves under the bf16 flag (img_bf16.hip diverts the others)
    assert cl.gemm_layers(0, "bf16", "conv") == ("0", "15", "17") and cl.gemm_layers(0, "bf16", "wgrad") == ("0", "10", "12", "15", "17")
    assert cl.gemm_layers(1, "bf16", "conv") == ("0", "14") and cl.gemm_layers(1, "bf16", "wgrad") == ("0", "8", "11", "14")
    assert all(cl.gemm_layers(k, "fp32", w) == cc.layer_names(k) for k in (0, 1, 2) for w in ("conv", "wgrad"))


def test_workspace_size_equals_the_library_s_at_every_batch():
    lib = var_amd.load_library()
    for kind in (0, 1, 2):
        bad = [B for B in range(1, cl.MAX_BATCH + 1) if 4 * cl.layout_total_floats(kind, B) != lib.var_convstack_workspace_bytes(kind, B)]
        assert not bad, (kind, bad[:8])


# ---- 2: the reduced references ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,R", [(0, 7, 3), (1, 15, 5), (2, 40, 5)])
def test_reduced_whole_stack_gradient_equals_the_full_float64_one(kind, B, R):
    P = cc.convstack_params(kind, 21)
    d = cl.repeated_data(kind, B, 21, R)
    full = cc.evaluate(kind, P, d, torch.float64)
    dsum = np.zeros((R, d["d_feat"].shape[1]))
    np.add.at(dsum, np.arange(B) % R, d["d_feat"].astype(np.float64))
    red = cc.evaluate(kind, P, {"image": d["distinct"], "d_feat": dsum}, torch.float64)
    worst = max((cc.rel(red[k], full[k]), k) for k in full if k.startswith("d."))
    print(f"kind {kind} B {B} R {R}: worst distance of the reduced from the full float64 gradient {worst[0]:.2e} at {worst[1]}")
    assert len([k for k in full if k.startswith("d.")]) == 2 * len(cc.layer_names(kind))
    assert worst[0] <= 1e-12
    for b in range(B):                                              # the copies' maps are the distinct images'
        assert np.array_equal(full["feat"][b], full["feat"][b % R])


@pytest.mark.parametrize("rounding", [False, True])
def test_reduced_layer_weight_gradient_equals_the_full_float64_one(rounding):
    kind, B, R, name = 0, 21, 4, "10"
    (_n, l, x_R, g), = cl.draw_layer_operands(kind, B, 5, (name,), rounding, R)
    _nm, _ci, cout, stride, pad, _pl = cb.geometry(kind)[l]
    assert not torch.equal(g[1], g[1 + R]) and float(g.abs().max()) > 0          # distinct g per copy
    full = cb.weight_grad(x_R[torch.arange(B) % R], g, (cout, x_R.shape[1], 3, 3), stride, pad, torch.float64, rounding).numpy()
    red = cl.reference(kind, l, x_R, g, R, rounding)
    err = cb.rel(red["d.10.weight"], full)
    print(f"rounding {rounding}: reduced against full float64 weight gradient {err:.2e}")
    assert err <= 1e-12
    assert cb.rel(red["d.10.bias"], g.double().sum((0, 2, 3)).numpy()) <= 1e-12


# ---- 3: the bound rejects injected faults -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,B,name", [(0, 148, "15"), (1, 92, "11")])
def test_the_bound_rejects_every_injected_fault_and_passes_the_clean_stand_in(kind, B, name):
    l = cc.layer_names(kind).index(name)
    (_n, _l, x_R, g), = cl.draw_layer_operands(kind, B, cl.LARGE_SEED, (name,), False)
    bound = cl.large_bounds(kind, B, (name,))
    ref = cl.reference(kind, l, x_R, g)
    assert set(bound) == set(ref) == {f"d.{name}.weight", f"d.{name}.weight.rowsum", f"d.{name}.weight.colsum", f"d.{name}.bias"}

    def ratios(fault):
        got = cl.standin(kind, l, x_R, g, fault)
        return {k: cb.rel(got[k], ref[k]) / bound[k] for k in ref}

    clean = ratios(None)
    print(f"kind {kind} B {B} layer {name}: bounds {({k: f'{v:.2g}' for k, v in bound.items()})}")
    print(f"  clean stand-in: error / bound {({k: f'{v:.3f}' for k, v in clean.items()})}")
    assert max(clean.values()) <= 1.0, clean
    # the faults sit where no batch of 25 or fewer reaches: a chunk and a slab beyond that size's last
    plan, small = cl.wgrad_plan(kind, l, B), cl.wgrad_plan(kind, l, cl.TESTED_BEFORE)
    assert (plan["splits"] - 2) * plan["per"] >= small["kchunks"] and plan["splits"] - 1 > small["splits"]
    for fault in cl.FAULTS:
        r = ratios(fault)
        weights = max(v for k, v in r.items() if "weight" in k)
        print(f"  {fault}: error / bound, weight arrays {weights:.3g}, bias {r[f'd.{name}.bias']:.3g}")
        if fault == "drop_bias_chunk":
            assert r[f"d.{name}.bias"] > 1.0 and weights <= 1.0, r
        elif fault == "shifted_copy":
            assert r[f"d.{name}.bias"] > 1.0 and r[f"d.{name}.weight"] > 1.0, r
        else:
            assert r[f"d.{name}.weight"] > 1.0 and r[f"d.{name}.bias"] <= 1.0, r


# ---- 4: the kernels' own order of additions -------------------------------------------------------------------------------------------------
def test_the_emulations_add_what_they_should():
    r = np.random.default_rng(3)
    g = r.integers(-8, 9, size=(3, 70001)).astype(np.float32)       # small integers: every order of additions is exact
    part = cl.emulate_chan_sum(g)
    assert part.shape == (cl.CHAN_CHUNKS, 3) and np.array_equal(cl.emulate_fold(part), g.astype(np.float64).sum(1))
    slabs = r.integers(-8, 9, size=(1020, 37)).astype(np.float32)
    assert np.array_equal(cl.emulate_fold(slabs), slabs.astype(np.float64).sum(0))
    assert np.array_equal(cl.emulate_fold_wide(slabs[:128]), slabs[:128].astype(np.float64).sum(0))
    x = np.ones((17, 1), dtype=np.float32)                          # and the order is the stated one: slabs 0 and 16 share a chain
    x[0, 0], x[16, 0] = 2.0 ** 24, -2.0 ** 24                       # and cancel there; in slab order the ones between them are lost
    assert cl.emulate_fold(x)[0] == 15.0 and cl.emulate_fold_wide(x)[0] == 0.0


@pytest.mark.parametrize("B", [400, 1024])
def test_bias_sum_and_fold_in_their_own_order_at_the_update_s_lengths(B):
    """Prints, for a 96 x 96 map at batch B with the test inputs' distribution (a Gaussian g gated to half its units), the distance
    from float64 of cs_chan_sum_kernel + cs_fold_kernel in their own order next to torch's fp32 sum, and the same for the fold of
    conv 1's weight-gradient slabs: the figures a miss on the GPU is judged against."""
    C, inner = 4, 96 * 96
    g = cl.gaussian((B, C, 96, 96), 7).numpy()
    g *= np.random.default_rng(8).random(g.shape) < 0.5
    ref = g.astype(np.float64).sum((0, 2, 3))
    emu = cl.emulate_fold(cl.emulate_chan_sum(np.ascontiguousarray(g.reshape(B, C, inner).transpose(1, 0, 2)).reshape(C, -1)))
    tor = torch.from_numpy(g).sum((0, 2, 3)).numpy()
    d_emu, d_tor = cb.rel(emu, ref), cb.rel(tor, ref)
    print(f"B {B}: bias sum of a 96 x 96 map, threads add {cl.chan_sum_chain(0, 0, B)} elements: own order {d_emu:.2e}, torch {d_tor:.2e} "
          f"of the largest magnitude from float64")
    assert d_emu < 1e-4 and d_tor < 1e-4
    # conv 1's slabs: split s holds the sum over its pixels of g * x for every output (16 of the 864 here), x a byte / 255
    plan = cl.wgrad_plan(0, 0, B)
    K, n_out = B * inner, 16
    gk = g[:, 0].reshape(-1).astype(np.float64)
    starts = np.arange(plan["splits"]) * plan["per"] * cl.WGRAD_KC
    assert starts[-1] < K and plan["splits"] == cl.wgrad_split(0, 0, B)
    r = np.random.default_rng(9)
    slabs = np.stack([np.add.reduceat(gk * (r.integers(0, 256, size=K) / 255.0), starts) for _ in range(n_out)], 1).astype(np.float32)
    ref = slabs.astype(np.float64).sum(0)
    d_emu, d_tor = cb.rel(cl.emulate_fold(slabs), ref), cb.rel(torch.from_numpy(slabs).sum(0).numpy(), ref)
    print(f"B {B}: fold of conv 1's {plan['splits']} slabs as 16 chains of {-(-plan['splits'] // 16)}: own order {d_emu:.2e}, torch {d_tor:.2e}")
    assert d_emu < 1e-4 and d_tor < 1e-4


# ---- 5: the gather-GEMM's accumulator chain ------------------------------------------------------------------------------------------------
def test_the_chain_emulations_compute_the_convolution_and_its_transpose():
    g = torch.Generator().manual_seed(2)
    ints = lambda *s: torch.randint(-3, 4, s, generator=g).float()   # noqa: E731  (small integers: every order is exact)
    for stride, pad, h in ((1, 1, 6), (2, 1, 7), (2, 0, 12), (1, 0, 5)):
        x, w, b = ints(2, 5, h, h), ints(4, 5, 3, 3), ints(4)
        assert torch.equal(cl.chain_conv_forward(x, w, b, stride, pad).double(), cb.conv_forward(x, w, b, stride, pad, torch.float64, False))
    for pad, h in ((1, 6), (0, 5)):
        gy, w = ints(2, 4, h + 2 * pad - 2, h + 2 * pad - 2), ints(4, 5, 3, 3)
        assert torch.equal(cl.chain_data_grad(gy, w, pad).double(), cb.data_grad(gy, w, (2, 5, h, h), 1, pad, torch.float64, False))
    # on real operands: the distances the three rows are held to (torch's blocked sums give 1.4e-6, 1.1e-6 and 1.3e-6 as four
    # distances on the same operands: convstack_bf16_cpu.bounds(kind, 4, rounding=False))
    for kind in (0, 1):
        chain = cl.chain_bounds(kind)
        print(f"kind {kind}: four distances of the chain order from float64 {({r: f'{v:.3g}' for r, v in chain.items()})}")
        assert set(chain) == set(cl.CHAIN_ROWS[kind]) and all(1e-6 < v < 1e-5 for v in chain.values())

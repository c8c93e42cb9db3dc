"""GPU checks of the PPO update's recurrent sequence (csrc/gru_seq.hip: var_gru_seq_fwd / var_gru_seq_bwd; var_amd.masked_gru /
forward_gru / bind_forward_gru) against the float64 checker of tests/gru_seq_cpu.py and the fixture made from the reference's
NNBase._forward_gru (tests/golden/gru_seq_t7.npz).

Bounds are measured, not chosen (gru_seq_cpu.gru_distance): per output array four times the distance of torch's own fp32 CPU
evaluation of the segmented nn.GRU form from float64, the largest over 20 seeded draws at the tested shape, relative to the
array's largest magnitude.  Against the fixture -- the reference's own fp32 numbers, themselves up to one such distance from
float64 -- the bound is five distances (triangle inequality).  Every test prints what it measured.  Mask structure, chaining,
determinism, graph replay and the binding are bit for bit."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import gru_seq_cpu as gc

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 4, 64), (3, 2, 128, 512), (3, 2, 128, 1024), (5, 16, 128, 512), (4, 17, 20, 64), (7, 5, 128, 512)]
# (T, N, I, H) that first run a path of csrc/gru_seq.hip's tiling.  A wave's share of a step's product is H/64 k-steps of 16 forward
# and 3H/64 backward, taken 8, then 4, then 1 at a time (mac_all); the shapes above give 1 | 8 | 16 and 3 | 24 | 48.
TILING_SHAPES = [
    (2, 3, 8, 256),        # forward 4 alone, backward 8 + 4
    (2, 3, 8, 320),        # forward 4 + 1, backward 8 + 4 + 1 + 1 + 1
    (2, 33, 129, 128),     # three env blocks, the last with one env; a second M tile of one row in d_x and d_w_ih; 1 + 1 | 4 + 1 + 1
    (1, 64, 1024, 64),     # both upper limits at once, and T = 1
    (2, 48, 1, 192),       # I = 1 (a reduction of one k); backward 8 + 1
    (3, 17, 128, 1024),    # a ragged second env block at the iTHOR hidden size
    (2, 16, 20, 64),       # 32 rows: the last size on the batched products' 32-column tile
    (3, 11, 20, 64),       # 33 rows: the first on the 64-column tile
]
SHAPES += TILING_SHAPES    # every shape's bounds: 20 draws (gru_seq_cpu.gru_distance)
KEYS = ("x", "hxs", "masks", "w_ih", "w_hh", "b_ih", "b_hh")
SENT = -77.0


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


@pytest.fixture(scope="module")
def ctx(var_amd):
    from var_amd._lib import Context
    return Context.get(0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def run(var_amd, d, with_dhT=None):
    """masked_gru on the GPU; with_dhT None: forward only, else also the six gradients of sum(out * d_out) (+ sum(h_T * d_hT))."""
    t = {k: dev(d[k]) for k in KEYS}
    leaves = [t[k].requires_grad_() for k in KEYS if k != "masks"] if with_dhT is not None else []
    out, h_T = var_amd.masked_gru(*(t[k] for k in KEYS))
    res = {"out": host(out), "h_T": host(h_T)}
    if with_dhT is not None:
        obj = (out * dev(d["d_out"])).sum()
        if with_dhT:
            obj = obj + (h_T * dev(d["d_hT"])).sum()
        g = torch.autograd.grad(obj, leaves)
        res.update({k: host(v) for k, v in zip(gc.GRADS, g)})
    return res


_REF = {}


def reference(shape, golden_dir):
    """(inputs, float64 results without d_hT, with d_hT) of a shape, computed once and shared."""
    if shape not in _REF:
        d = gc.load_fixture(golden_dir)[0] if shape == gc.FIXTURE_SHAPE else gc.gru_inputs(*shape, seed=100 + sum(shape))
        _REF[shape] = (d,) + gc.evaluate(d, torch.float64, "steps", both=True)
    return _REF[shape]


def check(got, ref, bounds, keys, what):
    worst = {k: gc.rel(got[k], ref[k]) for k in keys}
    print(what, {k: (f"{worst[k]:.3g}", f"bound {bounds[k]:.3g}") for k in keys})
    ratio = {k: worst[k] / bounds[k] if bounds[k] else (0.0 if worst[k] == 0 else np.inf) for k in keys}
    top = max(keys, key=ratio.get)
    print(f"{what}: worst error / bound {ratio[top]:.3f} at {top}")
    for k in keys:
        assert np.isfinite(got[k]).all(), k
        assert worst[k] <= bounds[k], (what, k, worst[k], bounds[k])


# ---- 1, 2, 3: parity within measured bounds ----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
def test_forward_matches_float64(var_amd, golden_dir, shape):
    d, ref, _ = reference(shape, golden_dir)
    got = run(var_amd, d)
    print("torch fp32 distances", shape, {k: gc.gru_distance(*shape)[False][k] for k in gc.OUTPUTS})
    check(got, ref, gc.gru_bounds(*shape, False), gc.OUTPUTS, f"forward {shape}")
    N = shape[1]
    assert np.array_equal(bits(got["h_T"]), bits(got["out"][-N:]))


@pytest.mark.parametrize("with_dhT", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_backward_matches_float64_autograd(var_amd, golden_dir, shape, with_dhT):
    d, r0, r1 = reference(shape, golden_dir)
    got = run(var_amd, d, with_dhT)
    print("torch fp32 distances", shape, with_dhT, {k: gc.gru_distance(*shape)[with_dhT][k] for k in gc.GRADS})
    check(got, r1 if with_dhT else r0, gc.gru_bounds(*shape, with_dhT), gc.GRADS, f"backward {shape} d_hT={with_dhT}")


@pytest.mark.parametrize("with_dhT", [False, True])
def test_fixture_from_the_reference(var_amd, golden_dir, with_dhT):
    d, g = gc.load_fixture(golden_dir)
    got = run(var_amd, d, with_dhT)
    dist = gc.fixture_distances(got, g, with_dhT)
    bounds = {k: 5.0 * v for k, v in gc.gru_distance(*gc.FIXTURE_SHAPE)[with_dhT].items()}
    print("vs the reference fixture", {k: (f"{dist[k]:.3g}", f"bound {bounds[k]:.3g}") for k in dist})
    assert set(dist) == set(gc.OUTPUTS + gc.GRADS)
    for k, v in dist.items():
        assert v <= bounds[k], (k, v, bounds[k])


# ---- 4: mask structure, exact ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape, t0, n0", [((5, 16, 128, 512), 2, 3), ((4, 17, 20, 64), 3, 16), ((3, 2, 128, 1024), 1, 0)])
def test_a_zero_mask_cuts_the_history_exactly(var_amd, shape, t0, n0):
    T, N, I, H = shape
    d = gc.gru_inputs(*shape, seed=77)
    m = d["masks"].reshape(T, N)
    m[:] = 1.0
    m[t0, n0] = 0.0
    a = run(var_amd, d)
    e = {k: v.copy() for k, v in d.items()}
    e["hxs"][n0] = np.random.default_rng(1).normal(size=H).astype(np.float32)
    e["x"].reshape(T, N, I)[:t0, n0] = np.random.default_rng(2).normal(size=(t0, I)).astype(np.float32)
    b = run(var_amd, e)
    oa, ob = a["out"].reshape(T, N, H), b["out"].reshape(T, N, H)
    assert np.array_equal(bits(oa[t0:, n0]), bits(ob[t0:, n0]))
    assert not np.array_equal(oa[:t0, n0], ob[:t0, n0])             # (the replaced history did matter before the cut)
    others = [n for n in range(N) if n != n0]
    assert np.array_equal(bits(oa[:, others]), bits(ob[:, others]))
    d["d_out"].reshape(T, N, H)[:t0, n0] = 0.0
    for with_dhT in (False, True):
        g = run(var_amd, d, with_dhT)
        assert (g["d_hxs"][n0] == 0.0).all() and (g["d_x"].reshape(T, N, I)[:t0, n0] == 0.0).all()
        assert np.abs(g["d_x"].reshape(T, N, I)[t0:, n0]).min() > 0 and (N == 1 or np.abs(g["d_hxs"][others]).max() > 0)


# ---- 5: chaining -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 16, 128, 512), (4, 17, 20, 64)])
def test_one_call_equals_chained_single_steps(var_amd, shape):
    T, N, I, H = shape
    d = gc.gru_inputs(*shape, seed=31)
    whole = run(var_amd, d)
    t = {k: dev(d[k]) for k in KEYS}
    h, outs = t["hxs"], []
    for s in range(T):
        o, h = var_amd.masked_gru(t["x"][s * N:(s + 1) * N], h, t["masks"][s * N:(s + 1) * N], t["w_ih"], t["w_hh"], t["b_ih"], t["b_hh"])
        outs.append(o)
    assert np.array_equal(bits(host(torch.cat(outs))), bits(whole["out"]))
    assert np.array_equal(bits(host(h)), bits(whole["h_T"]))


# ---- 6: determinism -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 16, 128, 512), (4, 17, 20, 64), (3, 2, 128, 1024)] + TILING_SHAPES[:2])
def test_two_runs_give_equal_bits(var_amd, shape):
    d = gc.gru_inputs(*shape, seed=13)
    a, b = run(var_amd, d, True), run(var_amd, d, True)
    for k in gc.OUTPUTS + gc.GRADS:
        assert np.array_equal(bits(a[k]), bits(b[k])), k


# ---- 7: graph capture ---------------------------------------------------------------------------------------------------------
def test_forward_and_backward_replay_from_a_captured_graph(var_amd):
    from var_amd._lib import new_graph
    shape = (4, 17, 20, 64)
    names = KEYS + ("d_out", "d_hT")
    draws = [gc.gru_inputs(*shape, seed=200 + i) for i in range(4)]
    eager = [run(var_amd, d, True) for d in draws]                  # (also creates the context before the capture)
    static = {k: dev(draws[0][k]) for k in names}
    leaves = [static[k].requires_grad_() for k in KEYS if k != "masks"]
    g = new_graph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.graph(g, stream=side):
        out, h_T = var_amd.masked_gru(*(static[k] for k in KEYS))
        obj = (out * static["d_out"]).sum() + (h_T * static["d_hT"]).sum()
        grads = torch.autograd.grad(obj, leaves)
    torch.cuda.current_stream().wait_stream(side)
    for i in (1, 2, 3):
        with torch.no_grad():
            for k in names:
                static[k].copy_(dev(draws[i][k]))
        g.replay()
        got = {"out": host(out), "h_T": host(h_T)}
        got.update({k: host(v) for k, v in zip(gc.GRADS, grads)})
        for k in gc.OUTPUTS + gc.GRADS:
            assert np.array_equal(bits(got[k]), bits(eager[i][k])), (i, k)


# ---- 8: the binding -----------------------------------------------------------------------------------------------------------
def test_a_bound_base_returns_what_masked_gru_returns(var_amd):
    T, N, I, H = 4, 3, 20, 64
    d = gc.gru_inputs(T, N, I, H, seed=8)
    base = gc.StandInBase(I, H).cuda()
    assert var_amd.bind_forward_gru(base) is base
    p = (base.gru.weight_ih_l0, base.gru.weight_hh_l0, base.gru.bias_ih_l0, base.gru.bias_hh_l0)
    x, hxs, masks = dev(d["x"]), dev(d["hxs"]), dev(d["masks"])
    for rows in (T * N, N):                                        # the sequence branch, the single-step branch
        a = base._forward_gru(x[:rows], hxs, masks[:rows])
        b = var_amd.masked_gru(x[:rows], hxs, masks[:rows], *p)
        c = var_amd.forward_gru(base.gru, x[:rows], hxs, masks[:rows])
        assert a[0].shape == (rows, H) and a[1].shape == (N, H)
        for u, v, w in zip(a, b, c):
            assert np.array_equal(bits(host(u)), bits(host(v))) and np.array_equal(bits(host(u)), bits(host(w)))


def test_ppo_loss_through_a_bound_actor_critic_fills_every_gradient(var_amd):
    """var_amd.PPO.loss on a stand-in (GRU + two Linear layers + DiagGaussian) whose base runs the op: every parameter's
    gradient against the same module in float64 on the CPU, within four times torch fp32's own distance (20 draws)."""
    import copy
    T, N, I, H, n = 5, 4, 20, 64, 2
    p64 = gc.StandInPolicy(I, H, n, seed=3).double()
    s = gc.ppo_sample(p64, T, N, I, n, seed=4)
    ref = gc.ppo_param_grads(p64, s, torch.float64)
    pol = var_amd.bind_forward_gru(copy.deepcopy(p64).float().cuda())
    agent = var_amd.PPO(pol, gc.CLIP, 1, 1, gc.VCOEF, gc.ECOEF, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    total, vl, al, ent = agent.loss(gc.sample_tuple(s, dev))
    agent.optimizer.zero_grad()
    total.backward()
    with torch.no_grad():
        t64 = float(gc.ppo_total(p64, gc.sample_tuple(s, lambda a: torch.from_numpy(a).double())))
    print("total", float(total.detach()), "float64", t64)
    dist = gc.ppo_distance(T, N, I, H, n)
    got = {k: v.grad for k, v in pol.named_parameters()}
    assert set(got) == set(ref) and len(ref) == 9
    for k in ref:
        assert got[k] is not None, k
        w, bound = gc.rel(host(got[k]), ref[k]), gc.MARGIN * dist[k]
        print(k, f"{w:.3g}", f"bound {bound:.3g}")
        assert np.abs(ref[k]).max() > 0 and w <= bound, (k, w, bound)


# ---- 9: error paths -------------------------------------------------------------------------------------------------------------
def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def test_refused_calls_leave_the_outputs_untouched(ctx):
    lib = ctx.lib

    def attempt(T, N, I, H, ws_short=False, alias=None, direction="fwd"):
        Hs, Is, Ns, Ts = max(H, 64), max(I, 1), max(N, 1), max(T, 1)
        f = lambda *s: torch.full(s, SENT, device="cuda")           # noqa: E731
        x, hxs, masks = f(Ts * Ns, Is), f(Ns, Hs), torch.ones(Ts * Ns, 1, device="cuda")
        w_ih, w_hh, b_ih, b_hh = f(3 * Hs, Is), f(3 * Hs, Hs), f(3 * Hs), f(3 * Hs)
        out, h_T, saved = f(Ts * Ns, Hs), f(Ns, Hs), f(5, Ts * Ns, Hs)
        # the workspace of the nearest shape the library accepts, doubled: room for whatever a wrongly accepted call would touch
        need = 2 * lib.var_gru_seq_workspace_bytes(Ts, min(Ns, 64), min(Is, 1024), min(1024, (Hs + 63) // 64 * 64))
        assert need > 0
        ws = torch.full((need // 4 + 4,), SENT, device="cuda")
        nbytes = need
        if ws_short:                                               # one word short of gi (forward) / one granule short (backward)
            nbytes = 4 * Ts * Ns * 3 * Hs - 4 if direction == "fwd" else need // 2 - 256
        outs = [out, h_T, saved, ws]
        if direction == "fwd":
            o = {"x": x, "hxs": hxs}.get(alias, out)
            rc = lib.var_gru_seq_fwd(ctx.handle, None, p(x), p(hxs), p(masks), p(w_ih), p(w_hh), p(b_ih), p(b_hh), T, N, I, H,
                                     p(o), p(h_T), p(saved), p(ws), nbytes)
            outs += [x, hxs]
        else:
            g = [f(Ts * Ns, Is), f(Ns, Hs), f(3 * Hs, Is), f(3 * Hs, Hs), f(3 * Hs), f(3 * Hs)]
            rc = lib.var_gru_seq_bwd(ctx.handle, None, p(x), p(masks), p(w_ih), p(w_hh), p(saved), p(out), None, T, N, I, H,
                                     *(p(t) for t in g), p(ws), nbytes)
            outs += g
        torch.cuda.synchronize()
        assert rc == -1, (T, N, I, H, ws_short, alias, direction, rc)
        assert lib.var_last_error(ctx.handle).decode().startswith("var_gru_seq_" + direction)
        for t in outs:
            assert (t == SENT).all()

    for direction in ("fwd", "bwd"):
        for T, N, I, H in ((2, 3, 8, 96), (2, 3, 8, 1088), (2, 3, 8, 0), (2, 3, 0, 64), (2, 3, 1025, 64), (2, 0, 8, 64),
                           (2, 65, 8, 64), (0, 3, 8, 64)):
            attempt(T, N, I, H, direction=direction)
        attempt(2, 3, 8, 64, ws_short=True, direction=direction)
    attempt(2, 3, 64, 64, alias="x")                               # out on top of x (same size: I = H)
    attempt(1, 3, 8, 64, alias="hxs")                              # out on top of hxs (T = 1: same size)
    # and a good call right after the refused ones
    T, N, I, H = 2, 3, 8, 64
    d = gc.gru_inputs(T, N, I, H, seed=1)
    t = {k: dev(d[k]) for k in KEYS}
    out, h_T = torch.empty(T * N, H, device="cuda"), torch.empty(N, H, device="cuda")
    need = lib.var_gru_seq_workspace_bytes(T, N, I, H)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    rc = lib.var_gru_seq_fwd(ctx.handle, None, *(p(t[k]) for k in KEYS), T, N, I, H, p(out), p(h_T), None, p(ws), need)
    assert rc == 0
    ref = gc.evaluate(d, torch.float64, "steps")
    assert gc.rel(host(out), ref["out"]) < 1e-5

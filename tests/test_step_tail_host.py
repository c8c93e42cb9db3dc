"""The float64 restatements and yardsticks of tests/step_tail_cpu.py, held to their sources on the CPU: adam64 to
torch.optim.Adam in double and to the reference's three-step trajectory, graph_walk to tests/_oracle_ctx.py, triplet64 to
torch.nn.TripletMarginLoss in double -- and the comparison helpers of tests/test_gpu_step_tail.py to three planted errors."""
import os

import numpy as np
import pytest
import torch

from tests import step_tail_cpu as st
from tests._oracle_ctx import _Lib

# the shapes of tests/test_gpu_step_tail.py
ADAM_SIZES = {"host": (1, 255, 256, 257, 524288, 524289), "dev": (1, 63, 64, 65, 1023, 1024, 1025, 262144, 262145, 263205)}
ADAM_RAGGED = {"host": 257, "dev": 1025}
COUNTER_SIZES = (5000, 100, 300000, 1)
TRIPLET_B = (1, 63, 64, 65, 255, 256, 257, 1000)
TRIPLET_EXTRA = [(65, 0.2, 1.0), (65, 5.0, 100.0), (257, 0.2, 100.0), (257, 5.0, 100.0)]       # (B, margin, magnitude)
INBATCH_SHAPES = ((1, 1), (1, 2), (3, 63), (4, 64), (5, 65), (64, 1), (257, 130), (300, 70))
INBATCH_TAUS = [(5, 65, 0.01), (5, 65, 1.0), (257, 130, 0.01), (257, 130, 1.0)]


def rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


# ---- adam64 -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", [1, 2, 1000, 100000])
@pytest.mark.parametrize("h", st.HYPERS[1:4], ids=lambda h: f"wd{h.wd}-b{h.b1}")
def test_adam64_is_torch_adam_in_double(h, step):
    inp = st.adam_inputs(4097, 5 + step, "general", h.wd)
    for k in "gmv":
        inp[k][inp["planted"]["nan"]] = 1.0                      # (the NaN has its own test on the GPU)
    arrs = [inp[k].astype(np.float64) for k in "pgmv"]
    for c in (h, st.carried(h)):                                 # the decimal hyper-parameters and the ones a C float carries
        c = c._replace(step=step)
        want = st.adam_torch(*arrs, c.step, c.lr, c.b1, c.b2, c.eps, c.wd, torch.float64)
        p1, m1, v1, u = st.adam64(*arrs, c.step, c.lr, c.b1, c.b2, c.eps, c.wd)
        for name, a, b in (("m", m1, want[1]), ("v", v1, want[2])):
            assert np.abs(a - b).max() <= 1e-14 * np.abs(b).max(), name
        # the update, by its own size (p - p' loses digits of u to p): |u_torch - u| <= 1e-14 |u| + an ulp of p in double
        ut = arrs[0] - want[0]
        assert (np.abs(ut - u) <= 1e-14 * np.abs(u) + 2 * np.spacing(np.abs(arrs[0]))).all()
        assert np.array_equal(p1, arrs[0] - u)


def test_adam64_follows_the_reference_trajectory(golden_dir):
    """tests/golden/kuka_adam.npz holds the reference's parameters after 1 and 3 steps (fp32) but not its gradients, so the
    gradients come from the CPU network in double (oracle.torch_oracle.CPUTrainer) and adam64 takes the three steps beside
    torch's own double Adam: equal to 1e-12 of the step, and within the fixture's fp32 resolution of the reference."""
    from oracle.torch_oracle import CPUTrainer
    sd = dict(np.load(os.path.join(golden_dir, "kuka_weights.npz")))
    fx = dict(np.load(os.path.join(golden_dir, "kuka_adam.npz")))
    torch.set_num_threads(1)
    tr = CPUTrainer(sd, lr=1e-4, weight_decay=1e-6, dtype=torch.float64)
    names = [k for k, _ in tr.model.named_parameters()]
    flat = lambda get: np.concatenate([get(k).reshape(-1) for k in names])                  # noqa: E731
    params = dict(tr.model.named_parameters())
    p = flat(lambda k: params[k].detach().numpy().copy())
    m, v = np.zeros_like(p), np.zeros_like(p)
    for s in range(3):
        tr.step(torch.from_numpy(fx[f"image{s}"]), torch.from_numpy(fx[f"pos{s}"]), torch.from_numpy(fx[f"neg{s}"]))
        g = flat(lambda k: params[k].grad.numpy())
        # (torch's step s + 1 has used the gradient at torch's parameters; they agree with p to 1e-12 of a step, see below)
        p, m, v, _ = st.adam64(p, g, m, v, s + 1, 1e-4, 0.9, 0.999, 1e-8, 1e-6)
        pt = flat(lambda k: params[k].detach().numpy())
        assert (np.abs(p - pt) <= 1e-12 * 1e-4 + 2 * np.spacing(np.abs(pt))).all(), s
        p = pt.copy()
        if s in (0, 2):
            ref = flat(lambda k: fx[f"step{s + 1}." + k])
            # the fixture is the reference's fp32 run, and near this initialisation fp32 rounding of a gradient of eps' size
            # moves its whole update: the share of the arena test_fused_loss_grad_and_adam_vs_fixture asks of the GPU
            diff = np.abs(p - ref)
            print(f"step {s + 1}: {np.mean(diff < 2e-6):.5f} of the arena within 2e-6 of the fixture, max {diff.max():.2e}")
            assert np.mean(diff < 2e-6) > 0.995, s


def test_planted_adam_errors_exceed_the_bounds_tenfold():
    """What the GPU test would say to three wrong kernels: their float64 results, rounded to fp32, go through the GPU test's
    comparison in place of the device's."""
    n = 5000
    r32 = lambda a: a.astype(np.float32)                                                     # noqa: E731

    def variant(inp, c, wd=None, eps_inside=False, t=None):
        p, g, m, v = (inp[k].astype(np.float64) for k in "pgmv")
        wd = c.wd if wd is None else wd
        t = c.step if t is None else t
        g1 = g + wd * p
        m1 = m + (g1 - m) * (1 - c.b1)
        v1 = c.b2 * v + (1 - c.b2) * g1 * g1
        bc2s = np.sqrt(1 - c.b2 ** t)
        denom = (np.sqrt(v1) + c.eps) / bc2s if eps_inside else np.sqrt(v1) / bc2s + c.eps
        return r32(p - (c.lr / (1 - c.b1 ** t)) * m1 / denom), r32(m1), r32(v1)

    # the right kernel passes its own comparison (the rounding to fp32 alone)
    for h in st.HYPERS[:3]:
        hz = h._replace(wd=0.0)
        inp = st.adam_inputs(n, 9, "zero")
        d, D = st.adam_distances(inp, hz, *variant(inp, st.carried(hz))), st.adam_distance(n, hz, "zero")
        assert all(d[k] <= 4 * D[k] for k in d), (d, D)
        inp = st.adam_inputs(n, 9, "general", h.wd)
        assert st.adam_p_excess(inp, h, variant(inp, st.carried(h))[0], st.adam_update_distance(n, h)) <= 1.0
    # 1. the weight decay ignored: at 1e-6 (row 2 of the table) and at 0.1 (row 3), general form
    for h in st.HYPERS[1:3]:
        inp = st.adam_inputs(n, 9, "general", h.wd)
        got = variant(inp, st.carried(h), wd=0.0)
        d, D = st.adam_distances(inp, h, *got), st.adam_distance(n, h, "general")
        x = st.adam_p_excess(inp, h, got[0], st.adam_update_distance(n, h))
        print(f"wd {h.wd} ignored: m {d['m']:.2e} (bound {4 * D['m']:.2e}), v {d['v']:.2e} (bound {4 * D['v']:.2e}), p excess {x:.2e}")
        assert d["m"] >= 40 * D["m"] and d["v"] >= 40 * D["v"] and x >= 10.0
    # 2. eps added before the division by sqrt(bc2), 3. bias corrections of step t - 1: row 2 (step 3), p = 0 form
    h = st.HYPERS[1]._replace(wd=0.0)
    inp = st.adam_inputs(n, 9, "zero")
    D = st.adam_distance(n, h, "zero")
    for what, kw in (("eps inside", dict(eps_inside=True)), ("t - 1", dict(t=h.step - 1))):
        d = st.adam_distances(inp, h, *variant(inp, st.carried(h), **kw))
        print(f"{what}: u {d['u']:.2e} (bound {4 * D['u']:.2e})")
        assert d["u"] >= 40 * D["u"], what
        assert d["m"] <= 4 * D["m"] and d["v"] <= 4 * D["v"]              # (the moments are untouched by either)


def test_adam_inputs_hold_what_they_promise():
    for form, wd in (("zero", 0.0), ("general", 0.1)):
        inp = st.adam_inputs(5000, 3, form, wd)
        pl, g, m, v, p = inp["planted"], inp["g"], inp["m"], inp["v"], inp["p"]
        assert len(set(pl.values())) == 4
        assert g[pl["zero"]] == 0 and v[pl["zero"]] == 0 and m[pl["zero"]] == 0
        assert g[pl["eps"]] == np.float32(1e-8) and np.isnan(g[pl["nan"]]) and np.isnan(g).sum() == 1
        assert g[pl["cancel"]] == np.float32(-9) * m[pl["cancel"]]
        ok = ~np.isnan(g)
        assert (v >= 0).all() and (np.abs(g[ok & (g != 0)]) >= 9e-10).all() and np.abs(g[ok]).max() <= 90.0
        assert (p == 0).all() if form == "zero" else p.std() > 0.05
        w = st.f32(wd) * p.astype(np.float64)
        rest = np.ones(5000, bool)
        rest[list(pl.values())] = False
        assert (np.abs(g + w) >= 0.5 * (np.abs(g) + np.abs(w)))[rest].all()
    assert st.adam_inputs(1, 3, "zero")["planted"] == {} and len(st.adam_inputs(4, 3, "zero")["planted"]) == 4


# ---- graph_walk -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_rows, row_ints, ahead", [(1, 5, 0), (1, 5, 1), (2, 80, 1), (3, 1023, 0), (3, 1025, 1), (4, 3000, 1)])
def test_graph_walk_is_the_oracle_contexts(n_rows, row_ints, ahead):
    r = np.random.default_rng(n_rows * row_ints)
    table = r.integers(0, 1 << 30, (n_rows, row_ints)).astype(np.int32)
    lib = _Lib()
    n = 7
    arrs = [np.ascontiguousarray(r.normal(size=n).astype(np.float32)) for _ in range(4)]
    arrs[3] = np.abs(arrs[3])
    lr, step = np.array([1e-4], np.float32), np.array([0], np.int32)
    ptr = lambda a: a.ctypes.data                                                            # noqa: E731
    for start in (n_rows - 1, n_rows - 2):
        cur = np.array([start], np.int32)
        row = np.full(2 * row_ints, -5, np.int32)
        mine = start
        for launch in range(2):
            want_row, mine = st.graph_walk(table, mine, ahead)
            lib.var_adam_step_graph(None, None, *(ptr(a) for a in arrs), n, ptr(lr), 0.9, 0.999, 1e-8, 0.0, ptr(step), ptr(table),
                                    row_ints, n_rows, ptr(cur), ptr(row), ahead)
            assert int(cur[0]) == mine and np.array_equal(row[:want_row.size], want_row)
            assert want_row.size == (2 if ahead else 1) * row_ints and (row[want_row.size:] == -5).all()
    assert int(step[0]) == 4


# ---- triplet64 --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, margin, mag", [(1, 1.0, 1.0), (7, 1.0, 1.0), (65, 0.2, 1.0), (65, 5.0, 100.0), (257, 0.2, 100.0)])
def test_triplet64_is_torch_triplet_margin_loss_in_double(B, margin, mag):
    a, p, n, kind = st.triplet_inputs(B, 21, margin, mag)
    assert (kind == st.ZERO_DIST).sum() == (B >= 2) and ((kind == st.INACTIVE).sum() > 0) == (B >= 3)
    inv = 1.0 / (2 * B)
    got = st.triplet64(a, p, n, margin, inv)

    def module(eps):
        t = [torch.from_numpy(x).double().requires_grad_() for x in (a, p, n)]
        loss = torch.nn.TripletMarginLoss(margin=margin, p=2, eps=eps, reduction="sum")(*t) * inv
        loss.backward()
        return float(loss.detach()), [x.grad.numpy() for x in t]

    loss, grads = module(st.PD_EPS)
    assert abs(float(got["loss"][0]) - loss) <= 1e-14 * abs(loss)
    for k, g in zip(("ga", "gp", "gn"), grads):
        assert np.abs(got[k] - g).max() <= 1e-14 * inv, k
    # the decimal 1e-6 differs from the fp32 operation's float32(1e-6) by 2.5e-15: nothing, except on the zero-distance row
    loss6, grads6 = module(1e-6)
    rest = kind != st.ZERO_DIST
    assert abs(loss6 - loss) <= 1e-12 * abs(loss)
    for k, g in zip(("ga", "gp", "gn"), grads6):
        assert np.abs(got[k] - g)[rest].max(initial=0.0) <= 1e-9 * inv, k
    # inactive rows: exactly zero; the zero-distance row: the positive's gradient is 0, the anchor's is the negative's negated
    for k in ("ga", "gp", "gn"):
        assert (got[k][kind == st.INACTIVE] == 0).all() and (got[k][kind == st.ACTIVE] != 0).any(axis=1).all()
    if B >= 2:
        z = B // 2
        assert (((a[z] - p[z]) + np.float32(1e-6)) == 0).all()                            # exactly 0 in fp32
        assert (got["gp"][z] == 0).all() and np.array_equal(got["ga"][z], -got["gn"][z]) and (got["gn"][z] != 0).any()
        t32 = st.triplet_torch(a, p, n, margin, inv, torch.float32)                          # ... as torch's fp32 gives
        assert (t32["gp"][z] == 0).all() and np.array_equal(t32["ga"][z], -t32["gn"][z])


def test_inbatch_inputs_and_reference():
    a, cand, t = st.inbatch_inputs(257, 130, 4)
    assert t[0] == 0 and t[1] == 129 and t[2] == t[3] and np.array_equal(a[256], cand[t[256]])
    assert np.abs(np.linalg.norm(a, axis=1) - 1).max() < 1e-6
    ref = st.inbatch64(a, cand, t, 0.1, 1.0 / 257)
    # the closed form: softmax over the negative distances minus the one-hot target, by hand
    A, C = a.astype(np.float64), cand.astype(np.float64)
    u = A[:, None, :] - C[None, :, :] + 1e-6
    d = np.linalg.norm(u, axis=2)
    z = -d / 0.1
    lse = np.log(np.exp(z - z.max(1, keepdims=True)).sum(1)) + z.max(1)
    loss = (lse + d[np.arange(257), t] / 0.1).sum() / 257
    s = np.exp(z - lse[:, None])
    s[np.arange(257), t] -= 1.0
    w = (-s / 0.1 / 257 / d)[:, :, None] * u
    assert abs(ref["loss"][0] - loss) <= 1e-12 * loss
    assert rel(ref["ga"], w.sum(1)) <= 1e-10 and rel(ref["gc"], -w.sum(0)) <= 1e-10
    one = st.inbatch64(*st.inbatch_inputs(64, 1, 4), 0.1, 1.0 / 64)                         # M = 1: nothing to tell apart
    assert one["loss"][0] == 0 and (one["ga"] == 0).all() and (one["gc"] == 0).all()


# ---- the yardsticks ---------------------------------------------------------------------------------------------------------
def _finite_positive(d):
    return all(np.isfinite(x) and 0 < x < 1e-4 for x in d.values())


def test_adam_yardsticks_are_finite_and_deterministic():
    for kern, sizes in ADAM_SIZES.items():
        for h in st.HYPERS[:2]:
            for n in sizes:
                if n > 300000 and h is not st.HYPERS[0]:
                    continue                                     # (the large sizes once here: they take a second each)
                assert _finite_positive(st.adam_distance(n, h._replace(wd=0.0), "zero")), (n, h)
                assert _finite_positive(st.adam_distance(n, h, "general")), (n, h)
        for h in st.HYPERS[2:]:
            n = ADAM_RAGGED[kern]
            assert _finite_positive(st.adam_distance(n, h._replace(wd=0.0), "zero")) and _finite_positive(st.adam_distance(n, h, "general"))
    for t, (n, lr) in enumerate(zip(COUNTER_SIZES, (1e-4, 1e-4, 1e-5, 1e-5))):
        assert _finite_positive(st.adam_distance(n, st.HYPERS[0]._replace(lr=lr, step=t + 1), "zero"))
    first = dict(st.adam_distance(257, st.HYPERS[1], "general"))
    st.adam_distance.cache_clear()
    assert st.adam_distance(257, st.HYPERS[1], "general") == first


def test_head_yardsticks_are_finite_and_deterministic():
    cases = [(B, 1.0, 1.0 / B, 1.0) for B in TRIPLET_B] + [(B, mg, 1.0 / B, mag) for B, mg, mag in TRIPLET_EXTRA] + [(65, 1.0, 1.0 / 130, 1.0)]
    for c in cases:
        d = st.triplet_distance(*c)
        assert set(d) == {"loss", "ga", "gp", "gn"} and _finite_positive(d), (c, d)
        print(f"triplet {c}: " + ", ".join(f"{k} {x:.2e}" for k, x in sorted(d.items())))
    for B, M, tau in [(B, M, 0.1) for B, M in INBATCH_SHAPES] + INBATCH_TAUS:
        d = st.inbatch_distance(B, M, tau, 1.0 / B)
        assert set(d) == {"loss", "ga", "gc"} and all(np.isfinite(x) and 0 <= x < 1 for x in d.values()), (B, M, tau, d)
        assert M == 1 or all(x > 0 for x in d.values()), (B, M, tau, d)
        print(f"in-batch ({B},{M}) tau {tau}: " + ", ".join(f"{k} {x:.2e}" for k, x in sorted(d.items())))
    first = dict(st.triplet_distance(*cases[3])), dict(st.inbatch_distance(5, 65, 0.01, 0.2))
    st.triplet_distance.cache_clear()
    st.inbatch_distance.cache_clear()
    assert (st.triplet_distance(*cases[3]), st.inbatch_distance(5, 65, 0.01, 0.2)) == first

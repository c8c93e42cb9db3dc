"""GPU checks of the pretext step's tail, each kernel alone through the C ABI against the float64 restatements of
tests/step_tail_cpu.py: the three Adam entries (csrc/pack_adam.hip: adam_kernel behind var_adam_step, adam_pack_dev_kernel behind
var_adam_step_dev / var_adam_step_graph), the triplet loss (csrc/heads.hip: triplet_kernel) and the in-batch head
(csrc/inbatch.hip).  Every array sits between 64 sentinel elements on each side, and half of the Adam cases pass their arrays
one float past a 16-byte boundary.

Bounds.  No bound here is a constant: each is a half-ulp term of the fp32 format, or four times a distance of torch's own fp32
CPU evaluation of the same formulas from float64 -- the largest over 20 seeded draws at the tested shape and hyper-parameters,
per output array (step_tail_cpu.adam_distance / triplet_distance / inbatch_distance).  Adam's distances are elementwise ratios
against scales without cancellation (m: |m| + |g'|, v: v', update: S = (lr / bc1) (|m| + |g'|) / denom); the update is pinned by
the cases with p = 0 and wd = 0, where p' is the negated update and nothing else, and the general case (p ~ N(0, 0.1^2)) asks
|p_gpu - p64| <= max(ulp32(p), ulp32(p64)) / 2 + 4 D_u S -- which is what pins the weight decay.  The loss heads' distances are
relative to each array's largest magnitude.  All references take the hyper-parameters as the C floats the entries receive
(step_tail_cpu's docstring says why).
Seen on an MI355X, the largest distance over all cases beside the range of its bounds (the kernels sit at 0.2 .. 0.4 of them):
Adam, both kernels alike: m 6.1e-8 (bounds 1.0e-7 .. 2.3e-7), v 3.1e-7 (3.8e-7 .. 9.2e-7), update 3.2e-7 (1.8e-7 .. 1.2e-6), the
general form's |p - p64| over its bound 0.976 .. 1.000 of 1 (the half ulp of p' is the bound's larger part and is reached whenever
p' rounds by half an ulp).  Triplet: loss 9.7e-8 (3.0e-7 .. 2.1e-6), ga 2.6e-7, gp 1.9e-7, gn 1.3e-7 (4.0e-7 .. 1.1e-6).  In-batch
at tau 0.1 and 1: loss 1.6e-7 (3.7e-7 .. 6.2e-7), g_anchor 3.2e-7 (1.1e-6 .. 1.3e-6), g_cand 1.5e-7 (5.2e-7 .. 1.1e-6); at tau 0.01:
g_anchor 1.1e-6 (2.6e-6 .. 3.9e-6), g_cand 1.1e-6 (1.3e-6 .. 3.2e-6); M = 1: loss exactly 0 (9.5e-7, 3.8e-6).  (B, M) = (1, 2) is
the one loose case: among the 20 draws is an anchor next to its positive, whose loss of exp(-d/tau)'s size fp32 log-softmax cannot
resolve -- torch's own distance is 1e-2 .. 3e-2 there, the device's 1.5e-5 on the tested draw.

Not tested: an exact tie d(a,p) - d(a,n) + margin == 0 of the triplet loss.  The kernel counts it inactive where clamp_min
would pass the gradient on; the reference cannot reach it by construction (torch refuses margin 0), and an fp32 tie cannot be
planted robustly against the compiler's contraction of the sums of squares.  include/var_hip.h states the kernel's choice.
Targets of the in-batch head always lie inside [0, M): the host cannot refuse others, and no test tries them."""
import ctypes

import numpy as np
import pytest
import torch

from tests import step_tail_cpu as st

pytestmark = pytest.mark.gpu

SENT = -77.0
PAD = 64
ERR_ARG = -1
ADAM_SIZES = {"host": (1, 255, 256, 257, 524288, 524289), "dev": (1, 63, 64, 65, 1023, 1024, 1025, 262144, 262145, 263205)}
ADAM_RAGGED = {"host": 257, "dev": 1025}
N_PARAMS = 213478


@pytest.fixture(scope="module")
def ctx():
    import var_amd  # noqa: F401
    from var_amd._lib import Context
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return Context.get(0)


class Buf:
    """n elements between PAD sentinels on each side; shift = 1 starts them one element past a 16-byte boundary."""

    def __init__(self, data=None, n=None, dtype=torch.float32, shift=0):
        if data is not None:
            data = np.ascontiguousarray(data).reshape(-1)
            n = data.size
        self.n, self.lo = n, PAD + shift
        self.t = torch.full((self.lo + n + PAD,), SENT if dtype.is_floating_point else int(SENT), dtype=dtype, device="cuda")
        assert self.t.data_ptr() % 16 == 0
        if data is not None:
            self.t[self.lo:self.lo + n] = torch.from_numpy(data).cuda()
        self.before = self.t.clone()

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + self.lo * self.t.element_size())

    def host(self):
        torch.cuda.synchronize()
        return self.t[self.lo:self.lo + self.n].cpu().numpy().copy()

    def pads_ok(self):
        torch.cuda.synchronize()
        w = self.t.cpu().numpy()
        return bool((w[:self.lo] == SENT).all() and (w[self.lo + self.n:] == SENT).all())

    def untouched(self):
        """Bit for bit what it was made with, sentinels included."""
        torch.cuda.synchronize()
        return np.array_equal(bits(self.t.cpu().numpy()), bits(self.before.cpu().numpy()))


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def last_error(ctx):
    return ctx.lib.var_last_error(ctx.handle).decode()


# ---- Adam -------------------------------------------------------------------------------------------------------------------
class Walk:
    """The index table, cursor and row buffer of var_adam_step_graph."""

    def __init__(self, n_rows, row_ints, ahead, cursor, seed=0):
        self.table_np = np.random.default_rng(seed).integers(0, 1 << 30, (n_rows, row_ints)).astype(np.int32)
        self.n_rows, self.row_ints, self.ahead = n_rows, row_ints, ahead
        self.table = Buf(self.table_np, dtype=torch.int32)
        self.cursor = Buf(np.array([cursor], np.int32), dtype=torch.int32)
        self.row = Buf(n=2 * row_ints, dtype=torch.int32)


def run_adam(ctx, entry, inp, h, shift=0, lr_dev=None, step_dev=None, walk=None):
    """One launch of `entry` ('host': var_adam_step, 'dev': var_adam_step_dev, 'graph': var_adam_step_graph) on fresh buffers
    holding inp.  The device entries get the step as step_dev = step - 1.  Returns the buffers."""
    b = {k: Buf(inp[k], shift=shift) for k in "pgmv"}
    n = inp["p"].size
    arrs = [b[k].ptr for k in "pgmv"]
    if entry == "host":
        rc = ctx.lib.var_adam_step(ctx.handle, None, *arrs, n, h.lr, h.b1, h.b2, h.eps, h.wd, h.step)
    else:
        if lr_dev is None:
            lr_dev = Buf(np.array([h.lr], np.float32))
            step_dev = Buf(np.array([h.step - 1], np.int32), dtype=torch.int32)
        b["lr_dev"], b["step_dev"] = lr_dev, step_dev
        if entry == "dev":
            rc = ctx.lib.var_adam_step_dev(ctx.handle, None, *arrs, n, lr_dev.ptr, h.b1, h.b2, h.eps, h.wd, step_dev.ptr)
        else:
            w = walk
            rc = ctx.lib.var_adam_step_graph(ctx.handle, None, *arrs, n, lr_dev.ptr, h.b1, h.b2, h.eps, h.wd, step_dev.ptr,
                                             w.table.ptr if w else None, w.row_ints if w else 0, w.n_rows if w else 0,
                                             w.cursor.ptr if w else None, w.row.ptr if w else None, w.ahead if w else 0)
    assert rc == 0, last_error(ctx)
    torch.cuda.synchronize()
    return b


def check_adam(inp, h, b, label, lr_zero=False):
    """Pads, the gradient's bits, the planted elements, and the distances from float64 beside their bounds."""
    n, form, pl = inp["p"].size, inp["form"], inp["planted"]
    assert all(b[k].pads_ok() for k in "pmv") and b["g"].untouched(), label
    if "step_dev" in b:
        assert b["step_dev"].pads_ok() and b["lr_dev"].untouched() and int(b["step_dev"].host()[0]) == h.step, label
    p, m, v = (b[k].host() for k in "pmv")
    if pl:
        for name, a in (("p", p), ("m", m), ("v", v)):           # the NaN gradient: that element of p, m, v and no other
            assert np.array_equal(np.flatnonzero(np.isnan(a)), [pl["nan"]]), (label, name)
        if h.wd == 0:
            assert bits(p)[pl["zero"]] == bits(inp["p"])[pl["zero"]], label
    else:
        assert not any(np.isnan(a).any() for a in (p, m, v)), label
    hy = h._replace(wd=0.0) if form == "zero" else h
    D = dict(st.adam_distance(n, hy, form))
    d = st.adam_distances(inp, h, p, m, v)
    if lr_zero:                                                  # p keeps its bits; m and v advance all the same
        ok = ~np.isnan(inp["g"])
        assert np.array_equal(bits(p)[ok], bits(inp["p"])[ok]), label
        d.pop("u", None)
    line = " ".join(f"{k} {d[k]:.2e}/{4 * D[k]:.2e}" for k in sorted(d))
    fails = [k for k in d if not d[k] <= 4 * D[k]]
    if form == "general" and not lr_zero:
        x = st.adam_p_excess(inp, h, p, st.adam_update_distance(n, h))
        line += f" |p - p64| / (ulp/2 + 4 D_u S) {x:.3f}/1"
        if not x <= 1.0:
            fails.append("p")
    print(f"{label} n={n} {form}: {line}")
    assert not fails, (label, fails, line)


def adam_case(ctx, entry, n, h, form, seed, shift):
    hh = h._replace(wd=0.0) if form == "zero" else h
    inp = st.adam_inputs(n, seed, form, hh.wd)
    check_adam(inp, hh, run_adam(ctx, entry, inp, hh, shift), f"{entry} {tuple(hh)}")


SIZE_CASES = [(e, n, r, f, (i + r) % 2) for e in ("host", "dev") for r in (0, 1) for i, n in enumerate(ADAM_SIZES[e])
              for f in ("zero", "general")]


@pytest.mark.parametrize("entry, n, row, form, shift", SIZE_CASES, ids=[f"{e}-{n}-row{r + 1}-{f}" for e, n, r, f, _ in SIZE_CASES])
def test_adam_against_float64_at_the_grid_edges(ctx, entry, n, row, form, shift):
    """adam_kernel: a lone thread, the ragged last block, 2048 blocks full and the first element of a block's second round.
    adam_pack_dev_kernel: a lone lane, a ragged last wave, a ragged last block, the first looped element, a looped ragged tail."""
    adam_case(ctx, entry, n, st.HYPERS[row], form, 100 + n % 1000 + row, shift)


@pytest.mark.parametrize("form", ["zero", "general"])
@pytest.mark.parametrize("row", [2, 3, 4])
@pytest.mark.parametrize("entry", ["host", "dev"])
def test_adam_against_float64_at_the_other_hyper_parameters(ctx, entry, row, form):
    adam_case(ctx, entry, ADAM_RAGGED[entry], st.HYPERS[row], form, 300 + row, row % 2)


@pytest.mark.parametrize("entry", ["host", "dev", "graph"])
def test_adam_with_lr_zero_keeps_p_and_advances_the_moments(ctx, entry):
    h = st.HYPERS[1]._replace(lr=0.0)
    inp = st.adam_inputs(1025, 41, "general", h.wd)
    check_adam(inp, h, run_adam(ctx, entry, inp, h, 1), f"{entry} lr=0", lr_zero=True)


def test_adam_device_counter_and_learning_rate_across_grid_sizes(ctx):
    """Four launches on one step_dev / lr_dev with 5, 1, 256 and 1 blocks; the learning rate is rewritten between the second and
    the third.  A done_ctr that did not rewind would stop the single-block launches from counting."""
    lr_dev = Buf(np.array([1e-4], np.float32))
    step_dev = Buf(np.array([0], np.int32), dtype=torch.int32)
    for t, (n, lr) in enumerate(zip((5000, 100, 300000, 1), (1e-4, 1e-4, 1e-5, 1e-5)), start=1):
        if t == 3:
            lr_dev.t[lr_dev.lo] = 1e-5
            lr_dev.before = lr_dev.t.clone()
        h = st.HYPERS[0]._replace(lr=lr, step=t)
        inp = st.adam_inputs(n, 50 + t, "zero")
        b = run_adam(ctx, "dev" if t % 2 else "graph", inp, h, t % 2, lr_dev, step_dev)
        check_adam(inp, h, b, f"launch {t}")                     # (asserts step_dev == t)
    assert int(step_dev.host()[0]) == 4 and step_dev.pads_ok()


@pytest.mark.parametrize("n", [1, 65, 1025, 263205])
def test_adam_dev_and_graph_are_one_kernel_and_every_entry_repeats_its_bits(ctx, n):
    h = st.HYPERS[1]
    inp = st.adam_inputs(n, 60 + n % 100, "general", h.wd)
    out = {}
    for entry in ("host", "dev", "graph", "graph+table"):
        walk = [Walk(3, 7, 1, 0) for _ in range(2)] if entry == "graph+table" else [None, None]
        runs = [run_adam(ctx, entry.split("+")[0], inp, h, 1, walk=w) for w in walk]
        out[entry] = [runs[0][k].host() for k in "pmv"]
        for a, k in zip(out[entry], "pmv"):
            assert np.array_equal(bits(a), bits(runs[1][k].host())), (entry, k)
    for other in ("graph", "graph+table"):
        for a, c, k in zip(out["dev"], out[other], "pmv"):
            assert np.array_equal(bits(a), bits(c)), (other, k)
    # (host-step and device-step entries are each held to float64 above, not to each other: pow against repeated squaring)


def test_adam_on_a_foreign_arena_leaves_the_bound_weight_image(ctx):
    """An arena of exactly VAR_N_PARAMS floats that is not the bound model's: no re-pack.  (And the bound one does re-pack.)"""
    from var_amd._lib import ptr
    g = torch.Generator().manual_seed(3)
    bound = (0.1 * torch.randn(N_PARAMS, generator=g)).cuda()
    w = ctx.new_weights()
    try:
        w.pack(bound)
        image = ctx.debug_buffer("wpack").clone()
        h = st.HYPERS[1]
        inp = st.adam_inputs(N_PARAMS, 70, "general", h.wd)
        for entry in ("host", "dev", "graph", "graph"):
            b = run_adam(ctx, entry, inp, h, 0, walk=Walk(2, 5, 1, 0) if entry == "graph" else None)
            assert not np.array_equal(bits(b["p"].host()), bits(inp["p"]))
            assert torch.equal(ctx.debug_buffer("wpack"), image), entry
        z = torch.zeros(N_PARAMS, device="cuda")
        lr, step = torch.full((1,), 1e-2, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")
        grad, m, v = torch.ones_like(z), z, z.clone()
        ctx.check(ctx.lib.var_adam_step_dev(ctx.handle, None, ptr(bound), ptr(grad), ptr(m), ptr(v), N_PARAMS, ptr(lr), 0.9, 0.999,
                                            1e-8, 0.0, ptr(step)), "var_adam_step_dev")
        assert not torch.equal(ctx.debug_buffer("wpack"), image)
    finally:
        ctx.check(ctx.lib.var_weights_bind(ctx.handle, None), "var_weights_bind")
        del w


@pytest.mark.parametrize("n_rows, row_ints, ahead", [(1, 5, 0), (1, 5, 1), (2, 80, 1), (3, 1023, 0), (3, 1025, 1), (4, 3000, 1)])
def test_adam_graph_cursor_walk(ctx, n_rows, row_ints, ahead):
    h = st.HYPERS[0]
    for n in (1, 5000):
        inp = st.adam_inputs(n, 80, "zero")
        for start in (n_rows - 1, n_rows - 2):
            w = Walk(n_rows, row_ints, ahead, start, seed=n_rows * row_ints)
            lr_dev, step_dev = Buf(np.array([h.lr], np.float32)), Buf(np.array([0], np.int32), dtype=torch.int32)
            cur = start
            for launch in (1, 2):
                run_adam(ctx, "graph", inp, h, 0, lr_dev, step_dev, w)
                want, cur = st.graph_walk(w.table_np, cur, ahead)
                row = w.row.host()
                assert np.array_equal(row[:want.size], want) and (row[want.size:] == int(SENT)).all(), (n, start, launch)
                assert w.row.pads_ok() and w.table.untouched(), (n, start, launch)
                assert int(w.cursor.host()[0]) == cur and w.cursor.pads_ok(), (n, start, launch)
                assert int(step_dev.host()[0]) == launch and step_dev.pads_ok() and lr_dev.untouched()


def test_adam_refusals_touch_nothing(ctx):
    h = st.HYPERS[0]
    inp = st.adam_inputs(100, 90, "general")
    b = {k: Buf(inp[k]) for k in "pgmv"}
    lr_dev, step_dev = Buf(np.array([h.lr], np.float32)), Buf(np.array([4], np.int32), dtype=torch.int32)
    w = Walk(2, 5, 1, 0)
    everything = list(b.values()) + [lr_dev, step_dev, w.table, w.cursor, w.row]
    hyp = (h.b1, h.b2, h.eps, h.wd)

    def call(entry, drop=None, n=100, step=1, lr=True, st_=True, table=True, cursor=True, row=True, row_ints=5, n_rows=2):
        arrs = [None if k == drop else b[k].ptr for k in "pgmv"]
        if entry == "var_adam_step":
            return ctx.lib.var_adam_step(ctx.handle, None, *arrs, n, h.lr, *hyp, step)
        dev = (lr_dev.ptr if lr else None, *hyp, step_dev.ptr if st_ else None)
        if entry == "var_adam_step_dev":
            return ctx.lib.var_adam_step_dev(ctx.handle, None, *arrs, n, *dev)
        return ctx.lib.var_adam_step_graph(ctx.handle, None, *arrs, n, *dev, w.table.ptr if table else None, row_ints, n_rows,
                                           w.cursor.ptr if cursor else None, w.row.ptr if row else None, 1)

    cases = [(e, dict(drop=k)) for e in ("var_adam_step", "var_adam_step_dev", "var_adam_step_graph") for k in "pgmv"]
    cases += [(e, dict(n=0)) for e in ("var_adam_step", "var_adam_step_dev", "var_adam_step_graph")]
    cases += [("var_adam_step", dict(step=0))]
    cases += [(e, kw) for e in ("var_adam_step_dev", "var_adam_step_graph") for kw in (dict(lr=False), dict(st_=False))]
    cases += [("var_adam_step_graph", kw) for kw in (dict(cursor=False), dict(row=False), dict(row_ints=0), dict(n_rows=0))]
    for entry, kw in cases:
        assert call(entry, **kw) == ERR_ARG, (entry, kw)
        assert last_error(ctx).startswith(entry + ":"), (entry, kw, last_error(ctx))
    assert all(x.untouched() for x in everything)
    assert call("var_adam_step_graph", table=False, cursor=False, row=False, row_ints=0, n_rows=0) == 0      # no table: plain _dev
    assert int(step_dev.host()[0]) == 5 and w.cursor.untouched() and w.row.untouched()


# ---- triplet loss -----------------------------------------------------------------------------------------------------------
def run_triplet(ctx, a, p, n, margin, inv, outs=("ga", "gp", "gn")):
    B = a.shape[0]
    b = {"a": Buf(a), "p": Buf(p), "n": Buf(n), "loss": Buf(n=1), "ga": Buf(n=3 * B), "gp": Buf(n=3 * B), "gn": Buf(n=3 * B)}
    rc = ctx.lib.var_triplet_fwd_bwd(ctx.handle, None, b["a"].ptr, b["p"].ptr, b["n"].ptr, B, margin, inv, b["loss"].ptr,
                                     *(b[k].ptr if k in outs else None for k in ("ga", "gp", "gn")))
    assert rc == 0, last_error(ctx)
    assert all(b[k].untouched() for k in "apn") and all(b[k].pads_ok() for k in ("loss", "ga", "gp", "gn"))
    return b


def check_triplet(ctx, B, margin, inv, mag, seed):
    a, p, n, kind = st.triplet_inputs(B, seed, margin, mag)
    b = run_triplet(ctx, a, p, n, margin, inv)
    got = {k: b[k].host().reshape(-1, 3) if k != "loss" else b[k].host() for k in ("loss", "ga", "gp", "gn")}
    ref = st.triplet64(a, p, n, st.f32(margin), st.f32(inv))
    D = st.triplet_distance(B, margin, inv, mag)
    d = {k: float(np.abs(got[k].astype(np.float64) - ref[k]).max()) / st.scale(ref[k]) for k in ref}
    print(f"triplet B={B} margin={margin} inv_count={inv:.3e} x{mag:g}: " + " ".join(f"{k} {d[k]:.2e}/{4 * D[k]:.2e}" for k in sorted(d)))
    for k in ("ga", "gp", "gn"):                                 # inactive rows: exactly zero
        assert (got[k][kind == st.INACTIVE] == 0).all(), k
    if B >= 2:                                                   # the zero-distance row
        z = B // 2
        assert (got["gp"][z] == 0).all() and np.array_equal(bits(got["ga"][z]), bits(-got["gn"][z])) and (got["gn"][z] != 0).any()
    assert all(d[k] <= 4 * D[k] for k in d), d
    b2 = run_triplet(ctx, a, p, n, margin, inv)
    assert all(np.array_equal(bits(b[k].host()), bits(b2[k].host())) for k in ("loss", "ga", "gp", "gn"))
    return a, p, n, b


@pytest.mark.parametrize("B", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_triplet_against_float64_at_the_wave_and_block_edges(ctx, B):
    check_triplet(ctx, B, 1.0, 1.0 / B, 1.0, 200 + B)


@pytest.mark.parametrize("B, margin, mag", [(65, 0.2, 1.0), (65, 5.0, 100.0), (257, 0.2, 100.0), (257, 5.0, 100.0)])
def test_triplet_margins_and_magnitudes(ctx, B, margin, mag):
    check_triplet(ctx, B, margin, 1.0 / B, mag, 300 + B)


def test_triplet_inv_count_and_null_gradient_outputs(ctx):
    B = 65
    a, p, n, full = check_triplet(ctx, B, 1.0, 1.0 / (2 * B), 1.0, 400)
    for drop in ("ga", "gp", "gn"):
        b = run_triplet(ctx, a, p, n, 1.0, 1.0 / (2 * B), outs=[k for k in ("ga", "gp", "gn") if k != drop])
        assert b[drop].untouched(), drop
        for k in ("loss", "ga", "gp", "gn"):
            assert k == drop or np.array_equal(bits(b[k].host()), bits(full[k].host())), (drop, k)
    b = run_triplet(ctx, a, p, n, 1.0, 1.0 / (2 * B), outs=())
    assert np.array_equal(bits(b["loss"].host()), bits(full["loss"].host())) and all(b[k].untouched() for k in ("ga", "gp", "gn"))


def test_triplet_refusals_touch_nothing(ctx):
    a, p, n, _ = st.triplet_inputs(7, 1, 1.0)
    b = {"a": Buf(a), "p": Buf(p), "n": Buf(n), "loss": Buf(n=1), "ga": Buf(n=21), "gp": Buf(n=21), "gn": Buf(n=21)}
    for name, kw in (("a", dict(a=None)), ("loss_out", dict(loss=None)), ("B", dict(B=0))):
        q = {k: (kw[k] if k in kw else x.ptr) for k, x in b.items()}
        rc = ctx.lib.var_triplet_fwd_bwd(ctx.handle, None, q["a"], q["p"], q["n"], kw.get("B", 7), 1.0, 1.0 / 7, q["loss"], q["ga"],
                                         q["gp"], q["gn"])
        assert rc == ERR_ARG and last_error(ctx).startswith("var_triplet_fwd_bwd:"), name
    assert all(x.untouched() for x in b.values())


# ---- in-batch head ----------------------------------------------------------------------------------------------------------
def run_inbatch(ctx, a, cand, t, tau, inv):
    B, M = a.shape[0], cand.shape[0]
    b = {"a": Buf(a), "c": Buf(cand), "t": Buf(t, dtype=torch.int32), "scratch": Buf(n=2 * B), "loss": Buf(n=1), "ga": Buf(n=3 * B),
         "gc": Buf(n=3 * M)}
    rc = ctx.lib.var_inbatch_loss_fwd_bwd(ctx.handle, None, b["a"].ptr, b["c"].ptr, b["t"].ptr, B, M, tau, inv, b["scratch"].ptr,
                                          b["loss"].ptr, b["ga"].ptr, b["gc"].ptr)
    assert rc == 0, last_error(ctx)
    assert all(b[k].untouched() for k in "act") and all(b[k].pads_ok() for k in ("scratch", "loss", "ga", "gc"))
    return {"loss": b["loss"].host(), "ga": b["ga"].host().reshape(B, 3), "gc": b["gc"].host().reshape(M, 3)}


def check_inbatch(ctx, B, M, tau, inv, seed):
    a, cand, t = st.inbatch_inputs(B, M, seed)
    got = run_inbatch(ctx, a, cand, t, tau, inv)
    assert all(np.isfinite(x).all() for x in got.values())
    ref = st.inbatch64(a, cand, t, st.f32(tau), st.f32(inv))
    if M == 1:
        # one candidate: softmax = 1, no gradient; the loss is d/tau - d/tau, zero within the rounding of d/tau
        d64 = np.linalg.norm(a.astype(np.float64) - cand.astype(np.float64) + st.PD_EPS, axis=1) / st.f32(tau)
        bound = 4 * 0.5 * float(st.ulp32(d64.max())) * B * st.f32(inv)
        print(f"in-batch ({B},{M}) tau={tau}: |loss| {abs(float(got['loss'][0])):.2e}/{bound:.2e}")
        assert ref["loss"][0] == 0 and abs(float(got["loss"][0])) <= bound
        assert (got["ga"] == 0).all() and (got["gc"] == 0).all()
    else:
        D = st.inbatch_distance(B, M, tau, inv)
        d = {k: float(np.abs(got[k].astype(np.float64) - ref[k]).max()) / st.scale(ref[k]) for k in ref}
        print(f"in-batch ({B},{M}) tau={tau} inv_count={inv:.3e}: " + " ".join(f"{k} {d[k]:.2e}/{4 * D[k]:.2e}" for k in sorted(d)))
        assert all(d[k] <= 4 * D[k] for k in d), d
    again = run_inbatch(ctx, a, cand, t, tau, inv)
    assert all(np.array_equal(bits(got[k]), bits(again[k])) for k in got)
    return a, cand, t, ref


@pytest.mark.parametrize("B, M", [(1, 1), (1, 2), (3, 63), (4, 64), (5, 65), (64, 1), (257, 130), (300, 70)])
def test_inbatch_against_float64_at_the_wave_and_block_edges(ctx, B, M):
    check_inbatch(ctx, B, M, 0.1, 1.0 / B, 500 + B + M)


@pytest.mark.parametrize("tau", [0.01, 1.0])
@pytest.mark.parametrize("B, M", [(5, 65), (257, 130)])
def test_inbatch_temperatures(ctx, B, M, tau):
    """tau = 0.01: logits down to -200, only the max-subtraction keeps expf finite."""
    check_inbatch(ctx, B, M, tau, 1.0 / B, 600 + B + M)


def test_inbatch_global_inv_count_and_row_split(ctx):
    B, M = 257, 130
    check_inbatch(ctx, 5, 65, 0.1, 1.0 / 20, 700)
    a, cand, t, ref = check_inbatch(ctx, B, M, 0.1, 1.0 / B, 701)
    parts = [run_inbatch(ctx, a[s], cand, t[s], 0.1, 1.0 / B) for s in (slice(0, 128), slice(128, B))]
    whole = {"loss": parts[0]["loss"].astype(np.float64) + parts[1]["loss"], "ga": np.concatenate([parts[0]["ga"], parts[1]["ga"]]),
             "gc": parts[0]["gc"].astype(np.float64) + parts[1]["gc"]}
    D = st.inbatch_distance(B, M, 0.1, 1.0 / B)
    d = {k: float(np.abs(whole[k].astype(np.float64) - ref[k]).max()) / st.scale(ref[k]) for k in ref}
    print("in-batch (257,130) as rows 0..127 + 128..256: " + " ".join(f"{k} {d[k]:.2e}/{4 * D[k]:.2e}" for k in sorted(d)))
    assert all(d[k] <= 4 * D[k] for k in d), d


def test_inbatch_refusals_touch_nothing(ctx):
    a, cand, t = st.inbatch_inputs(5, 9, 1)
    b = {"a": Buf(a), "c": Buf(cand), "t": Buf(t, dtype=torch.int32), "scratch": Buf(n=10), "loss": Buf(n=1), "ga": Buf(n=15), "gc": Buf(n=27)}
    order = ("a", "c", "t", "scratch", "loss", "ga", "gc")
    cases = [dict(tau=0.0), dict(B=0), dict(M=0)] + [{k: None} for k in order]
    for kw in cases:
        q = {k: (None if k in kw else b[k].ptr) for k in order}
        rc = ctx.lib.var_inbatch_loss_fwd_bwd(ctx.handle, None, q["a"], q["c"], q["t"], kw.get("B", 5), kw.get("M", 9), kw.get("tau", 0.1),
                                              0.2, q["scratch"], q["loss"], q["ga"], q["gc"])
        assert rc == ERR_ARG and last_error(ctx).startswith("var_inbatch_loss_fwd_bwd:"), kw
    assert all(x.untouched() for x in b.values())

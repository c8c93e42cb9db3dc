"""GPU checks of the PPO update's optimiser step: var_clip_adam_step (csrc/clip_adam.hip) alone through the C ABI against the
float64 restatement of tests/clip_adam_cpu.py, then var_amd.ClipAdam and PPO(..., fused_optimizer=True) on both actor-critics.
Every array of a table lies in one backing tensor between 64 sentinel elements (also between its segments), each segment at a
chosen distance from a 16-byte boundary.

Hyper-parameters: the reference's PPO values (clip_adam_cpu.LR, EPS, MAX_NORM: RLLr 6e-5, RLEps 1e-5, RLMaxGradNorm 0.5 of
Envs/ai2thor/config.py:74-76; Adam's default betas), steps 1 (moments zero), 2 and 1000 (moments random).  Clip cases: gradients
scaled to a norm of 4 x max_norm (clipped), of max_norm / 4 (coef = 1), and max_norm <= 0 (no norm launch, total_norm_out
untouched).

Bounds.  No bound here is a constant: each is four times the distance of torch's own fp32 CPU evaluation of the whole composite
(clip_grad_norm_, then optim.Adam) from float64 -- the largest over 20 seeded draws at the tested table, step and clip case, per
output (clip_adam_cpu.distance: total_norm relatively; m, v and the update by step_tail_cpu's scales without cancellation) -- or
the half-ulp term of the fp32 format for p, as step_tail_cpu does it.  m, v, total_norm and the update do not depend on p, so the
yardstick is taken once, in the form with p = 0 where p' is the negated update, and serves the general form (p ~ N(0, 0.1^2), the
policies' own parameters) as well.  All references take the hyper-parameters as the C floats the entry receives.
The policies' yardstick (20 draws over 3.6 and 5.5 million elements, evaluated in float64) is the slow part: five to nine
seconds per policy, once per session; the whole file runs in about 35 s beside an MI355X.

Seen on an MI355X, the largest distance over all cases of the entry alone beside the range of its bounds (test_largest_distances_seen
prints them): total_norm 6.6e-8 (bounds 0 -- a lone gradient of 2.0, exact on both sides -- .. 8.4e-5: torch's fp32 CPU norm
drifts with the length, 2e-5 at a million elements, the kernel's pairwise sums do not), m 6.1e-8 (2.3e-8 .. 8.5e-6), v 3.6e-7
(4.5e-7 .. 1.7e-4), update 2.6e-7 (1.0e-7 .. 7.1e-5), the general form's |p - p64| over its bound 0.993 .. 1.000 of 1 (the half ulp
of p' is the bound's larger part and is reached whenever p' rounds by half an ulp).  (The bounds' upper ends belong to the clipped
cases of long tables: there torch's own coefficient carries its norm's error into every g'.)  One step on the policies:
total_norm 5.8e-8 (bounds 3.1e-5, 1.6e-4), against PyTorch's clip_grad_norm_ on the twin 3.4e-7, m 1.9e-8 (3.2e-6, 1.6e-5), v 4.0e-7
(6.3e-5, 3.2e-4), |p - p64| over its bound 1.000 of 1; the halved learning rate: |u_half - u / 2| 0.667 of its bound.

Bit for bit: two calls on equal inputs; the same tensors as one merged segment, as VAR_OPT_MAX_SEGS + 1 and as 2 VAR_OPT_MAX_SEGS + 1
segments (one, two and three pairs of launches) -- p, m, v and total_norm; a torch.cuda.graph capture of ClipAdam.step() replayed
three times against three eager steps.  After every call the gradients and all sentinels are untouched and step_dev has advanced
by exactly one."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import clip_adam_cpu as ca
from tests import convstack_cpu as cc
from tests import trunk_cpu as tc

pytestmark = pytest.mark.gpu

SENT, PAD, ERR_ARG = -77.0, 64, -1
MAX_SEGS = 64                                                    # VAR_OPT_MAX_SEGS
BLOCK, ROUND, FULL = 256, 1024, 1 << 20                          # threads, elements per workgroup and round, elements of a full grid's round
RATIOS = {"clipped": 4.0, "coef1": 0.25, "noclip": None}


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


@pytest.fixture(scope="module")
def ctx(var_amd):
    from var_amd._lib import Context
    return Context.get(0)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def last_error(ctx):
    return ctx.lib.var_last_error(ctx.handle).decode()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


class Scalar:
    """One element between PAD sentinels."""

    def __init__(self, value, dtype=torch.float32):
        self.t = torch.full((2 * PAD + 1,), SENT if dtype.is_floating_point else int(SENT), dtype=dtype, device="cuda")
        self.t[PAD] = value
        self.before = host(self.t)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr() + PAD * 4)

    def value(self):
        return host(self.t)[PAD]

    def pads_ok(self):
        w = host(self.t)
        return bool((np.delete(w, PAD) == SENT).all())

    def untouched(self):
        return np.array_equal(bits(host(self.t)), bits(self.before))


class Arrays:
    """The p, g, m, v of a table of segments, one backing tensor per array.  shifts[k][i]: how many floats past a 16-byte boundary
    segment i of array k starts; gap = False lays the segments of every array end to end (one contiguous run)."""

    def __init__(self, lens, inp, shifts=None, gap=True):
        self.lens = tuple(int(n) for n in lens)
        self.off, self.t, self.before, self.mask = {}, {}, {}, {}
        for k in "pgmv":
            sh = [0] * len(self.lens) if shifts is None else shifts[k]
            offs, end = [], 0
            for i, n in enumerate(self.lens):
                if gap or i == 0:
                    o = -(-(end + PAD) // 4) * 4 + sh[i]
                else:
                    o = end
                offs.append(o)
                end = o + n
            w = np.full(end + PAD, SENT, np.float32)
            mask = np.zeros(w.size, bool)
            for o, part in zip(offs, ca.split(inp[k], self.lens)):
                w[o:o + part.size] = part
                mask[o:o + part.size] = True
            self.off[k], self.mask[k], self.before[k] = offs, mask, w
            self.t[k] = torch.from_numpy(w).cuda()
            assert self.t[k].data_ptr() % 16 == 0

    def table(self, merged=False):
        """The C table; merged (gap = False only): the whole run as one segment."""
        from var_amd._lib import OptSeg
        idx = [0] if merged else range(len(self.lens))
        rows = [OptSeg(*(self.t[k].data_ptr() + 4 * self.off[k][i] for k in "pgmv"), sum(self.lens) if merged else self.lens[i]) for i in idx]
        return (OptSeg * len(rows))(*rows), len(rows)

    def host(self, k):
        return host(self.t[k])[self.mask[k]]

    def pads_ok(self, k):
        return bool((host(self.t[k])[~self.mask[k]] == SENT).all())

    def untouched(self, k):
        return np.array_equal(bits(host(self.t[k])), bits(self.before[k]))


def call(ctx, table, n, h, lr_dev, step_dev, tn):
    c = ca.Hyper(*h)
    return ctx.lib.var_clip_adam_step(ctx.handle, None, table, n, 0.0 if c.max_norm is None else c.max_norm, lr_dev.ptr if lr_dev else None,
                                      c.b1, c.b2, c.eps, step_dev.ptr if step_dev else None, tn.ptr if tn else None)


def run(ctx, lens, inp, h, shifts=None, gap=True, merged=False):
    """One call on fresh buffers holding inp (step_dev = step - 1): (arrays, lr_dev, step_dev, total_norm_out)."""
    a = Arrays(lens, inp, shifts, gap)
    lr_dev, step_dev, tn = Scalar(h.lr), Scalar(h.step - 1, torch.int32), Scalar(SENT)
    table, n = a.table(merged)
    rc = call(ctx, table, n, h, lr_dev, step_dev, tn)
    assert rc == 0, last_error(ctx)
    torch.cuda.synchronize()
    return a, lr_dev, step_dev, tn


SEEN = {}


def check(lens, inp, h, ratio, out, label):
    """Sentinels, the gradient's bits, the step count, and the distances from float64 beside their bounds."""
    a, lr_dev, step_dev, tn = out
    assert all(a.pads_ok(k) for k in "pmv") and a.untouched("g"), label
    assert lr_dev.untouched() and step_dev.pads_ok() and int(step_dev.value()) == h.step and tn.pads_ok(), label
    if h.max_norm is None:
        assert tn.untouched(), label
    p, m, v = (a.host(k) for k in "pmv")
    assert not any(np.isnan(x).any() for x in (p, m, v)), label
    if sum(lens) >= 4:
        assert bits(p)[0] == bits(inp["p"])[0], label              # g = m = v = 0: p keeps its bits
    D = ca.distance(tuple(lens), h, "zero", ratio or 1.0)
    ref = ca.reference(inp, h)
    d = ca.distances(inp, h, tn.value(), p, m, v, ref)
    fails = [k for k in d if not d[k] <= 4 * D[k]]
    line = " ".join(f"{k} {d[k]:.2e}/{4 * D[k]:.2e}" for k in sorted(d))
    if inp["form"] == "general":
        x = ca.p_excess(inp, h, p, D["u"], ref)
        line += f" |p - p64| / (ulp/2 + 4 D_u S) {x:.3f}/1"
        d["p"] = x
        if not x <= 1.0:
            fails.append("p")
    for k, x in d.items():
        s = SEEN.setdefault(k, [0.0, np.inf, 0.0])
        b = 1.0 if k == "p" else 4 * D[k]
        SEEN[k] = [max(s[0], x), min(s[1], b), max(s[2], b)]
    print(f"{label} n={sum(lens)} segs={len(lens)} {inp['form']}: {line}")
    assert not fails, (label, fails, line)
    return tn.value(), p, m, v


# ---- segment lengths and alignments -------------------------------------------------------------------------------------------
SIZES = (1, 3, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, ROUND - 1, ROUND, ROUND + 1, FULL, FULL + 1)
ALIGN = {"aligned": "", "all+1": "pgmv", "g+1": "g", "p+1": "p", "m+1": "m", "v+1": "v"}


@pytest.mark.parametrize("align", list(ALIGN))
@pytest.mark.parametrize("n", SIZES)
def test_one_segment_against_float64_at_the_grid_edges(ctx, n, align):
    """A lone element, a ragged quad, a ragged wave, a workgroup's 256 threads and its round of 1024 elements with their
    neighbours, the full grid of 1024 workgroups, and one element more: every workgroup makes a second round.  Each length with
    all four arrays on a 16-byte boundary, all four one float past it, and each array alone one float past it (mixed alignment)."""
    h = ca.hyper(2)
    inp = ca.inputs((n,), 100 + n % 1000, "zero", h, RATIOS["clipped"])
    shifts = {k: [1 if k in ALIGN[align] else 0] for k in "pgmv"}
    check((n,), inp, h, RATIOS["clipped"], run(ctx, (n,), inp, h, shifts), f"one segment {align}")


# ---- tables -------------------------------------------------------------------------------------------------------------------
def mixed_lens(count, seed, big=None):
    r = np.random.default_rng(seed)
    lens = [int(x) for x in r.choice((1, 1, 1, 2, 3, 5, 7, 17, 64, 100, 255, 1023), count)]
    if big is not None:
        lens[count // 2] = big
    return tuple(lens)


def mixed_shifts(count, seed):
    r = np.random.default_rng(seed)
    return {k: [int(x) for x in r.integers(0, 4, count)] for k in "pgmv"}


TABLES = {"one": (ROUND + 1,), "max": mixed_lens(MAX_SEGS, 1), "max+1": mixed_lens(MAX_SEGS + 1, 2),
          "2max+1": mixed_lens(2 * MAX_SEGS + 1, 3, big=300001)}


@pytest.mark.parametrize("case", list(RATIOS))
@pytest.mark.parametrize("step", [1, 2, 1000])
@pytest.mark.parametrize("name", list(TABLES))
def test_tables_steps_and_clip_cases_against_float64(ctx, name, step, case):
    """One segment, a full launch's table, one segment more (two pairs of launches) and 129 segments of mixed tiny lengths around
    one of 300001 floats (three pairs; workgroups whose elements lie in two launches), every segment of every array at its own
    distance from a 16-byte boundary; p = 0 (pins the update) and p ~ N(0, 0.1^2)."""
    lens = TABLES[name]
    h = ca.hyper(step, None if RATIOS[case] is None else ca.MAX_NORM)
    for form in ("zero", "general"):
        inp = ca.inputs(lens, 200 + step, form, h, RATIOS[case] or 1.0)
        check(lens, inp, h, RATIOS[case], run(ctx, lens, inp, h, mixed_shifts(len(lens), 4)), f"table {name} step {step} {case}")


def test_largest_distances_seen():
    """(prints what the cases above saw, for the docstring)"""
    for k, (worst, lo, hi) in sorted(SEEN.items()):
        print(f"{k}: largest {worst:.2e}, bounds {lo:.2e} .. {hi:.2e}")


# ---- bit for bit ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, case", [("one", "clipped"), ("max+1", "coef1"), ("2max+1", "clipped"), ("2max+1", "noclip")])
def test_two_calls_and_every_cut_of_the_table_give_equal_bits(ctx, name, case):
    lens = TABLES[name]
    h = ca.hyper(2, None if RATIOS[case] is None else ca.MAX_NORM)
    inp = ca.inputs(lens, 300, "general", h, RATIOS[case] or 1.0)
    results = {}
    for label, kw in (("spread", dict(shifts=mixed_shifts(len(lens), 5))), ("spread again", dict(shifts=mixed_shifts(len(lens), 5))),
                      ("run", dict(gap=False)), ("merged", dict(gap=False, merged=True))):
        results[label] = check(lens, inp, h, RATIOS[case], run(ctx, lens, inp, h, **kw), f"{name} {case} {label}")
    if len(lens) > MAX_SEGS + 1:                                 # the same run cut into VAR_OPT_MAX_SEGS + 1 segments: two pairs of launches
        cuts = np.linspace(0, sum(lens), MAX_SEGS + 2).astype(np.int64)
        coarse = tuple(int(x) for x in np.diff(cuts))
        a = Arrays(coarse, inp, gap=False)
        lr_dev, step_dev, tn = Scalar(h.lr), Scalar(h.step - 1, torch.int32), Scalar(SENT)
        assert call(ctx, *a.table(), h, lr_dev, step_dev, tn) == 0, last_error(ctx)
        results["recut"] = (tn.value(),) + tuple(a.host(k) for k in "pmv")
        assert all(a.pads_ok(k) for k in "pmv") and a.untouched("g") and int(step_dev.value()) == h.step
    first = results["spread"]
    for label, got in results.items():
        for x, y, k in zip(first, got, ("total_norm", "p", "m", "v")):
            assert np.array_equal(bits(np.asarray(x, np.float32)), bits(np.asarray(y, np.float32))), (label, k)


def cuda_params(sizes, seed):
    """Parameters that are views of one arena, with static gradients that are views of two flat buffers (as bind_convs and
    bind_trunk leave them) and one gradient of its own."""
    g = torch.Generator().manual_seed(seed)
    flat = (0.1 * torch.randn(sum(sizes), generator=g)).cuda()
    ps, o = [], 0
    for n in sizes:
        ps.append(torch.nn.Parameter(flat[o:o + n]))
        o += n
    half = len(sizes) // 2
    bufs = [torch.randn(sum(sizes[:half]), generator=g).cuda(), torch.randn(sum(sizes[half:-1]), generator=g).cuda()]
    o = [0, 0]
    for i, p in enumerate(ps[:-1]):
        b = 0 if i < half else 1
        p.grad = bufs[b][o[b]:o[b] + p.numel()]
        o[b] += p.numel()
    ps[-1].grad = torch.randn(sizes[-1], generator=g).cuda()
    return flat, ps


def test_a_captured_step_replays_like_three_eager_steps(var_amd):
    from var_amd._lib import new_graph
    sizes = (864, 32, 9216, 1, 70000, 3, 128, 1)
    flat_a, ps_a = cuda_params(sizes, 7)
    flat_b, ps_b = cuda_params(sizes, 7)
    assert torch.equal(flat_a, flat_b)
    a = var_amd.ClipAdam(ps_a, lr=ca.LR, eps=ca.EPS, max_norm=ca.MAX_NORM)
    b = var_amd.ClipAdam(ps_b, lr=ca.LR, eps=ca.EPS, max_norm=ca.MAX_NORM)
    assert len(a._table()[0]) == 3                               # two flat gradient buffers and the lone gradient
    norms = [host(a.step()) for _ in range(3)]
    graph = new_graph()
    with torch.cuda.graph(graph):
        tn = b.step()
    assert b.step_count() == 0 and torch.equal(flat_b, cuda_params(sizes, 7)[0])       # (capture runs nothing)
    for i in range(3):
        graph.replay()
        assert np.array_equal(bits(host(tn)), bits(norms[i])), i
    assert a.step_count() == 3 and b.step_count() == 3
    for x, y in ((flat_a, flat_b), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq)):
        assert np.array_equal(bits(host(x)), bits(host(y)))
    assert not torch.equal(flat_a, cuda_params(sizes, 7)[0])
    assert float(norms[0]) == float(norms[1]) > ca.MAX_NORM        # (static gradients: the same norm every step)


# ---- error paths ----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(ctx):
    from var_amd._lib import OptSeg
    lens = (5, 100, 7)
    h = ca.hyper(5)
    inp = ca.inputs(lens, 400, "general", h, 4.0)
    a = Arrays(lens, inp)
    lr_dev, step_dev, tn = Scalar(h.lr), Scalar(4, torch.int32), Scalar(SENT)
    P = {k: [a.t[k].data_ptr() + 4 * o for o in a.off[k]] for k in "pgmv"}

    def rows(edit=None, count=3):
        r = [[P[k][i] for k in "pgmv"] + [lens[i]] for i in range(count)]
        if edit:
            edit(r)
        return (OptSeg * len(r))(*(OptSeg(*x) for x in r)), len(r)

    def setv(i, j, value):
        def edit(r):
            r[i][j] = value
        return edit

    nan = float("nan")
    cases = [("n_seg 0", dict(n=0)), ("n_seg 257", dict(n=257)), ("no lr_dev", dict(lr=None)), ("no step_dev", dict(step=None)),
             ("n 0", dict(edit=setv(1, 4, 0))), ("n -3", dict(edit=setv(2, 4, -3)))]
    cases += [(f"NULL {'pgmv'[j]}", dict(edit=setv(1, j, None))) for j in range(4)]
    cases += [(f"{'pgmv'[j]} off by two bytes", dict(edit=setv(0, j, P["pgmv"[j]][0] + 2))) for j in range(4)]
    cases += [(f"{name} {x}", dict(hy={name: x})) for name in ("b1", "b2") for x in (-0.1, 1.0, 1.5, nan)]
    cases += [("eps -1", dict(hy=dict(eps=-1e-8))), ("eps NaN", dict(hy=dict(eps=nan))), ("max_norm NaN", dict(hy=dict(max_norm=nan)))]
    # overlaps: a p on another segment's p, on its own m, on a g; an m on a v; two g ranges
    cases += [("p[1] = p[0]", dict(edit=setv(1, 0, P["p"][0]))), ("p[0] into m[0]", dict(edit=setv(0, 0, P["m"][0] + 8))),
              ("p[2] into g[1]", dict(edit=setv(2, 0, P["g"][1] + 40))), ("m[1] into v[1]", dict(edit=setv(1, 2, P["v"][1] + 4 * 99))),
              ("g[2] = g[1]", dict(edit=setv(2, 1, P["g"][1]))), ("v[0] into p[1]", dict(edit=setv(0, 3, P["p"][1] - 4)))]
    for label, kw in cases:
        hh = h._replace(**kw.get("hy", {}))
        table, n = rows(kw.get("edit"))
        rc = ctx.lib.var_clip_adam_step(ctx.handle, None, table, kw.get("n", n), hh.max_norm, lr_dev.ptr if kw.get("lr", 1) else None,
                                        hh.b1, hh.b2, hh.eps, step_dev.ptr if kw.get("step", 1) else None, tn.ptr)
        assert rc == ERR_ARG, label
        assert last_error(ctx).startswith("var_clip_adam_step:"), (label, last_error(ctx))
    assert ctx.lib.var_clip_adam_step(ctx.handle, None, None, 1, 0.5, lr_dev.ptr, 0.9, 0.999, 1e-5, step_dev.ptr, tn.ptr) == ERR_ARG
    assert last_error(ctx).startswith("var_clip_adam_step:")
    torch.cuda.synchronize()
    assert all(a.untouched(k) for k in "pgmv") and lr_dev.untouched() and step_dev.untouched() and tn.untouched()
    # p[0] ending exactly where p[1] would begin is no overlap, and total_norm_out may be NULL
    table, n = rows()
    assert ctx.lib.var_clip_adam_step(ctx.handle, None, table, n, 0.5, lr_dev.ptr, 0.9, 0.999, 1e-5, step_dev.ptr, None) == 0, last_error(ctx)
    assert int(step_dev.value()) == 5 and tn.untouched() and not a.untouched("p") and a.untouched("g")


def test_nan_and_inf_gradients_go_through_as_in_pytorch(ctx):
    """A NaN gradient makes the norm, the coefficient and with them every parameter NaN, as clip_grad_norm_ + Adam do; without
    a clip only its own element.  An Inf gradient: norm Inf, coef 0, NaN at the Inf element (Inf * 0) and a zero gradient elsewhere."""
    lens, h = (10, 300), ca.hyper(2)
    base = ca.inputs(lens, 500, "general", h, 4.0)
    for bad, clip in ((np.nan, True), (np.nan, False), (np.inf, True)):
        inp = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in base.items()}
        inp["g"][17] = bad
        hh = h if clip else h._replace(max_norm=None)
        a, lr_dev, step_dev, tn = run(ctx, lens, inp, hh)
        p = a.host("p")
        tp = ca.clip_adam_torch(*(ca.split(inp[k], lens) for k in "pgmv"), ca.carried(hh), torch.float32)
        want = np.concatenate(tp[1])
        assert np.array_equal(np.isnan(p), np.isnan(want)), (bad, clip)
        assert np.isnan(p[17]) and int(step_dev.value()) == 2 and a.untouched("g")
        if clip:
            assert (np.isnan(tn.value()) if np.isnan(bad) else np.isinf(tn.value())) and np.isnan(p).all() == bool(np.isnan(bad))
        else:
            assert int(np.isnan(p).sum()) == 1 and tn.untouched()


# ---- ClipAdam and PPO on the two actor-critics ------------------------------------------------------------------------------------
T, N = 2, 2                                                      # the smallest rollout
N_ACT = {0: 2, 1: 8}
BINDERS = ("bind_convs", "bind_trunk")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def real_policy(var_amd, kind, Q, binder):
    """An ArmNetPolicy / IthorNetPolicy with Q loaded, on the GPU, its base bound by `binder`."""
    pol = tc.drop_in_policy(kind, 0).to("cuda")
    with torch.no_grad():
        for k, v in pol.named_parameters():
            v.copy_(dev(Q[k]))
    assert pol._arena_intact()
    return getattr(var_amd, binder)(pol)


_SAMPLES = {}


def minibatch(kind):
    if kind not in _SAMPLES:
        Q = cc.policy_params(kind, 9, N_ACT[kind])
        _SAMPLES[kind] = (Q, cc.ppo_sample(kind, Q, T, N, N_ACT[kind], 41))
    return _SAMPLES[kind]


def sample_tuple(kind, s):
    obs = {k: dev(s[k]) for k in ("image", "image_feat", "goal_sound_feat") + (("occupancy",) if kind else ("robot_pose",))}
    return (obs,) + tuple(dev(s[k]) for k in ("hxs", "actions", "value_preds", "returns", "masks", "old_logp", "adv"))


def agent_of(var_amd, pol, fused, lr=ca.LR, epochs=1, batches=1):
    return var_amd.PPO(pol, tc.CLIP, epochs, batches, tc.VCOEF, tc.ECOEF, lr=lr, eps=ca.EPS, max_grad_norm=ca.MAX_NORM, fused_optimizer=fused)


def backward(agent, sample):
    agent.optimizer.zero_grad()
    agent.loss(sample)[0].backward()


def flat_of(pol, what):
    return np.concatenate([host(what(p)).reshape(-1) for p in pol.parameters()])


@pytest.mark.parametrize("binder", BINDERS)
@pytest.mark.parametrize("kind", [0, 1])
def test_one_step_of_clip_adam_on_a_policy_against_float64(var_amd, kind, binder):
    """Two copies of the policy, one minibatch, loss(sample)[0].backward() on both; the copy with ClipAdam takes one step and is
    held, parameter by parameter, to the float64 restatement evaluated on the OTHER copy's gradients, its total_norm to PyTorch's
    clip_grad_norm_ on that twin.  The yardstick is taken in the clip case the twin's float64 norm falls in.
    Through bind_convs every kernel of the backward is this library's, and the two copies' gradients must agree bit for bit.
    Through bind_trunk the convolution stacks run under PyTorch autograd, whose two backward passes differ on an MI355X (seen:
    norms 1.8e-6 apart), so the twin's gradients are not what the step consumed: there the restatement takes the stepping copy's
    own gradients, read before the step and shown bit for bit untouched after it -- the same check of the optimiser."""
    Q, s = minibatch(kind)
    sample = sample_tuple(kind, s)
    pol, twin = (real_policy(var_amd, kind, Q, binder) for _ in range(2))
    agent, other = agent_of(var_amd, pol, True), agent_of(var_amd, twin, False)
    assert isinstance(agent.optimizer, var_amd.ClipAdam) and isinstance(other.optimizer, torch.optim.Adam)
    backward(agent, sample)
    backward(other, sample)
    lens = tuple(p.numel() for p in pol.parameters())
    names = [k for k, _ in pol.named_parameters()]
    own, theirs = flat_of(pol, lambda p: p.grad), flat_of(twin, lambda p: p.grad)
    same = np.array_equal(bits(own), bits(theirs))
    print(f"kind {kind} {binder}: {len(lens)} tensors, {sum(lens)} elements, {len(agent.optimizer._table()[0])} segments; "
          f"the two copies' gradients {'agree bit for bit' if same else 'differ'}")
    assert same or binder == "bind_trunk"
    inp = {"p": flat_of(twin, lambda p: p.data), "g": theirs if same else own, "form": "general"}
    inp["m"] = inp["v"] = np.zeros_like(inp["p"])
    tn = host(agent.optimizer.step())
    tn_twin = float(torch.nn.utils.clip_grad_norm_(twin.parameters(), ca.MAX_NORM))
    assert np.array_equal(bits(flat_of(pol, lambda p: p.grad)), bits(own))               # the gradients are left as they are
    h = ca.hyper(1)
    ref = ca.reference(inp, h)
    ratio = RATIOS["clipped"] if ref["tn"] > ca.MAX_NORM else RATIOS["coef1"]
    D = ca.distance(lens, h, "zero", ratio)
    opt = agent.optimizer
    p, m, v = flat_of(pol, lambda p: p.data), host(opt.exp_avg), host(opt.exp_avg_sq)
    d = ca.distances(inp, h, tn, p, m, v, ref)
    d["tn vs twin"] = abs(float(tn) - tn_twin) / tn_twin
    D["tn vs twin"] = D["tn"]
    print("  " + " ".join(f"{k} {d[k]:.2e}/{4 * D[k]:.2e}" for k in sorted(d)) + f"  total_norm {float(tn):.6g} (float64 {ref['tn']:.6g}, twin {tn_twin:.6g})")
    assert all(d[k] <= 4 * D[k] for k in d), d
    o, worst = 0, (0.0, None)
    for name, n in zip(names, lens):
        worst = max(worst, (ca.p_excess(inp, h, p, D["u"], ref, slice(o, o + n)), name))
        o += n
    print(f"  |p - p64| / (ulp/2 + 4 D_u S): worst {worst[0]:.3f}/1 at {worst[1]}")
    assert worst[0] <= 1.0, worst
    assert opt.step_count() == 1 and pol._arena_intact()


class Box:                                       # stand-ins for gym.spaces: the storage reads __class__.__name__ and .shape / .n
    def __init__(self, n):
        self.shape = (n,)


class Discrete:
    def __init__(self, n):
        self.n = n


def filled_rollout(var_amd, kind):
    n_act = N_ACT[kind]
    shapes = {'image': (3, 96, 96), 'image_feat': (3,), 'goal_sound_feat': (3,)}
    shapes.update({'occupancy': (1, 9, 9)} if kind else {'robot_pose': (2,)})
    ro = var_amd.RolloutStorage(T, N, shapes, Discrete(n_act) if kind else Box(n_act), tc.hidden(kind), types.SimpleNamespace(RLObsIgnore=[]),
                                image_dtype=torch.uint8)
    g = torch.Generator().manual_seed(4)
    obs = None
    for _ in range(T):
        obs = {k: (torch.randint(0, 256, (N,) + tuple(sh), generator=g, dtype=torch.uint8) if k in ("image", "occupancy")
                   else torch.randn((N,) + tuple(sh), generator=g)).cuda() for k, sh in shapes.items()}
        act = torch.randint(0, n_act, (N, 1), generator=g) if kind else torch.randn(N, n_act, generator=g)
        ro.insert(obs, (0.5 * torch.randn(N, tc.hidden(kind), generator=g)).cuda(), act.cuda(), (torch.randn(N, 1, generator=g) * 0.3 - 1.5).cuda(),
                  torch.randn(N, 1, generator=g).cuda(), torch.randn(N, 1, generator=g).cuda(), (torch.rand(N, 1, generator=g) < 0.8).float().cuda(),
                  torch.ones(N, 1).cuda())
    ro.compute_returns(torch.randn(N, 1, generator=g).cuda(), True, 0.99, 0.95, True)
    return ro, obs


@pytest.mark.parametrize("binder", BINDERS)
@pytest.mark.parametrize("kind", [0, 1])
def test_ppo_update_with_the_fused_optimizer_trains_the_arena_the_acting_graph_reads(var_amd, kind, binder):
    Q, _ = minibatch(kind)
    pol = real_policy(var_amd, kind, Q, binder)
    ro, obs = filled_rollout(var_amd, kind)
    step = pol.capture(N, deterministic=True)
    masks = torch.ones(N, 1, device="cuda")
    before = step(obs, masks)[0].clone()
    step.reset()
    agent = agent_of(var_amd, pol, True, epochs=2, batches=2)
    stats = agent.update(ro)
    assert len(stats) == 3 and all(isinstance(x, float) and np.isfinite(x) for x in stats), stats
    assert agent.optimizer.step_count() == 4 and pol._arena_intact()
    after = step(obs, masks)[0].clone()
    eager = pol.act(obs, torch.zeros(N, tc.hidden(kind), device="cuda"), masks, deterministic=True)[0]
    print(f"kind {kind} {binder}: stats {stats}, value {host(before).ravel()} -> {host(after).ravel()}")
    assert not np.array_equal(bits(host(after)), bits(host(before)))
    assert np.array_equal(bits(host(after)), bits(host(eager)))
    plain = agent_of(var_amd, real_policy(var_amd, kind, Q, binder), False)
    assert isinstance(plain.optimizer, torch.optim.Adam) and not isinstance(plain.optimizer, var_amd.ClipAdam)


def test_a_moved_arena_is_refused(var_amd):
    Q, s = minibatch(0)
    pol = real_policy(var_amd, 0, Q, "bind_convs")
    agent = agent_of(var_amd, pol, True)
    backward(agent, sample_tuple(0, s))
    first = next(pol.parameters())
    first.data = first.data.clone()                              # (one parameter leaves the arena)
    before = host(pol._flat)
    with pytest.raises(var_amd.VarHipError, match="arena has moved"):
        agent.optimizer.step()
    assert np.array_equal(bits(host(pol._flat)), bits(before)) and agent.optimizer.step_count() == 0


@pytest.mark.parametrize("kind", [0, 1])
def test_update_linear_schedule_halves_the_next_update(var_amd, kind):
    """Two one-step runs from equal state, one with lr and one whose param_groups were set to lr / 2 after a first step's worth of
    construction (models/ppo/utils.py:45-49 at epoch = total / 2): the second's update is half the first's, within the update's
    bound on both."""
    Q, s = minibatch(kind)
    sample = sample_tuple(kind, s)
    runs = []
    for halve in (False, True):
        pol = real_policy(var_amd, kind, Q, "bind_convs")
        agent = agent_of(var_amd, pol, True)
        if halve:
            for group in agent.optimizer.param_groups:           # update_linear_schedule(optimizer, 1, 2, LR)
                group['lr'] = ca.LR - (ca.LR * (1 / float(2)))
        p0 = flat_of(pol, lambda p: p.data).astype(np.float64)
        backward(agent, sample)
        g = flat_of(pol, lambda p: p.grad)
        agent.optimizer.step()
        runs.append((p0, g, flat_of(pol, lambda p: p.data).astype(np.float64)))
    (p0, g, full), (q0, g2, half) = runs
    assert np.array_equal(p0, q0) and np.array_equal(bits(g), bits(g2))
    lens = tuple(p.numel() for p in pol.parameters())
    inp = {"p": p0.astype(np.float32), "g": g, "m": np.zeros_like(g), "v": np.zeros_like(g), "form": "general"}
    h = ca.hyper(1)
    ref = ca.reference(inp, h)
    ratio = RATIOS["clipped"] if ref["tn"] > ca.MAX_NORM else RATIOS["coef1"]
    D_u = ca.update_distance(lens, h, ratio)
    # each run's p' is within ulp/2 + 4 D_u S of its float64 value, and the float64 updates are u and u / 2 exactly (lr / 2 is
    # exact in fp32): |(p0 - half) - (p0 - full) / 2| <= 1.5 (ulp32(p) / 2 + 4 D_u S)
    bound = 1.5 * (0.5 * np.maximum(ca.st.ulp32(p0), ca.st.ulp32(ref["p"])) + 4.0 * D_u * ref["S"])
    err = np.abs((p0 - half) - (p0 - full) / 2)
    moved = np.abs(p0 - full) > 0
    print(f"kind {kind}: {int(moved.sum())} of {p0.size} parameters moved; worst |u_half - u / 2| / bound {float((err / bound).max()):.3f}")
    assert moved.sum() > p0.size // 4 and bool((err <= bound).all())
    assert float(np.abs(p0 - half).sum()) < 0.75 * float(np.abs(p0 - full).sum())

"""GPU checks of csrc/ppo_step.hip: var_ppo_head_linear (the distribution head's Linear fused with var_ppo_head's loss) against
the float64 restatement and the bounds of tests/ppo_head_linear_cpu.py, against var_ppo_head fed the returned head (bit for
bit), for equal bits, the extent of its writes, its cursor form and its refusals; var_rollout_move_cursor against
var_rollout_move.

Shapes.  A workgroup takes ROWS_PER_WG = 256 rows per round and rows are grid-strided over at most MAX_WG = 256 workgroups
(ppo_step.hip: kRowsWG, kMaxWG), so M = 255 / 256 / 257 are one workgroup short of full, full, and two workgroups, and
M_WRAP = 256 * 256 + 257 makes workgroups 0 and 1 take a second round, workgroup 1's a single row."""
import ctypes

import numpy as np
import pytest
import torch

from tests import ppo_head_linear_cpu as hl
from tests import rollout_cpu as rc

pytestmark = pytest.mark.gpu

ROWS_PER_WG, MAX_WG = 256, 256
M_WRAP = ROWS_PER_WG * MAX_WG + ROWS_PER_WG + 1
SMALL_M = (1, 2, ROWS_PER_WG - 1, ROWS_PER_WG, ROWS_PER_WG + 1)
HEADS = [(0, 1), (0, 2), (0, 4), (1, 1), (1, 2), (1, 8), (1, 16)]
SENT, GUARD = -77.0, 64                                          # guard floats on both sides of every output (256 bytes)


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
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


class Buffers:
    """Every output inside its own sentinel-filled allocation, GUARD floats on both sides."""

    def __init__(self, ctx, kind, n, M):
        self.ws_bytes = ctx.lib.var_ppo_head_linear_workspace_bytes(kind, n, M)
        assert self.ws_bytes > 0 and self.ws_bytes % 16 == 0
        sizes = {"head": M * n, "out": 4, "g_features": M * hl.F, "g_W": n * hl.F, "g_b": n, "g_value": M, "g_logstd": n,
                 "workspace": self.ws_bytes // 4}
        self.sizes = sizes
        self.full = {k: torch.full((v + 2 * GUARD,), SENT, device="cuda") for k, v in sizes.items()}
        self.view = {k: self.full[k][GUARD:GUARD + v] for k, v in sizes.items()}

    def guards_intact(self):
        torch.cuda.synchronize()
        return all(bool((f[:GUARD] == SENT).all()) and bool((f[GUARD + self.sizes[k]:] == SENT).all()) for k, f in self.full.items())

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((f == SENT).all()) for f in self.full.values())


def call(ctx, kind, t, clipped, n, M, buf, stats=None, n_stats=0, cursor=None, n_env=0, stream=None, over=None):
    a = dict(features=t["features"], W=t["W"], b=t["b"], logstd=t["logstd"], value=t["value"], action=t["action"],
             old_logp=t["old_logp"], adv=t["adv"], returns=t["returns"], value_preds=t["value_preds"], ws_bytes=buf.ws_bytes, kind=kind,
             n=n, M=M, clip=rc.CLIP, **buf.view)
    a.update(over or {})
    q = lambda x: x if x is None or isinstance(x, ctypes.c_void_p) else p(x)            # noqa: E731
    return ctx.lib.var_ppo_head_linear(ctx.handle, stream, a["kind"], q(a["features"]), q(a["W"]), q(a["b"]), q(a["logstd"]),
                                       q(a["value"]), q(a["action"]), q(a["old_logp"]), q(a["adv"]), q(a["returns"]),
                                       q(a["value_preds"]), a["n"], a["M"], a["clip"], rc.VCOEF, rc.ECOEF, int(clipped), q(a["head"]),
                                       q(a["out"]), q(a["g_features"]), q(a["g_W"]), q(a["g_b"]), q(a["g_value"]), q(a["g_logstd"]),
                                       q(a["workspace"]), a["ws_bytes"], q(stats), n_stats, q(cursor), n_env)


def plain_head(ctx, kind, t, head, clipped, n, M):
    """var_ppo_head on `head`: (out, g_head, g_value, g_logstd)."""
    out, g_head, g_value = torch.empty(4, device="cuda"), torch.empty(M, n, device="cuda"), torch.empty(M, device="cuda")
    g_logstd = torch.empty(n, device="cuda") if kind == 0 else None
    assert ctx.lib.var_ppo_head(ctx.handle, None, kind, p(head), p(t["logstd"]), p(t["value"]), p(t["action"]), p(t["old_logp"]),
                                p(t["adv"]), p(t["returns"]), p(t["value_preds"]), n, M, rc.CLIP, rc.VCOEF, rc.ECOEF, int(clipped),
                                p(out), p(g_head), p(g_value), p(g_logstd), None) == 0
    return out, g_head, g_value, g_logstd


def results(buf, kind):
    return {k: host(v) for k, v in buf.view.items() if k != "workspace" and (kind == 0 or k != "g_logstd")}


def check_case(ctx, kind, n, M, clipped, seed=1):
    d, redrawn = hl.inputs(kind, M, n, seed)
    assert redrawn * 10 <= M or redrawn <= 1, (redrawn, M)      # at most 1 draw in 10 (one row of a handful is allowed)
    assert not hl.near_kink(kind, d).any()
    t = {k: dev(v) for k, v in d.items()}
    buf = Buffers(ctx, kind, n, M)
    assert call(ctx, kind, t, clipped, n, M, buf) == 0
    assert buf.guards_intact()
    got = results(buf, kind)
    for k, a in got.items():
        assert not (a == SENT).any(), k                          # fully overwritten (no result is the sentinel)
    want, bound = hl.ref(kind, d, clipped), hl.bounds(kind, M, n, clipped)
    err = hl.errors(got, want)
    for k in err:
        print(f"HL_RATIO kind {kind} n {n} M {M} clipped {int(clipped)} {k} {err[k] / bound[k] if bound[k] else 0.0:.3f}")
    for k in err:
        assert err[k] <= bound[k], (k, err[k], bound[k])
    # var_ppo_head on the returned head: the same bits where both produce the array
    out, g_head, g_value, g_logstd = plain_head(ctx, kind, t, buf.view["head"].view(M, n), clipped, n, M)
    assert np.array_equal(bits(host(out)), bits(got["out"]))
    assert np.array_equal(bits(host(g_value)), bits(got["g_value"]))
    if kind == 0:
        assert np.array_equal(bits(host(g_logstd)), bits(got["g_logstd"]))
    gh = host(g_head).astype(np.float64)                         # g_head is not an output: its float64 products pin the rest
    via = {"g_features": gh @ d["W"].astype(np.float64), "g_W": gh.T @ d["features"].astype(np.float64), "g_b": gh.sum(0),
           "scales": want["scales"]}
    for k, e in hl.errors({k: got[k] for k in via if k != "scales"}, via).items():
        assert e <= bound[k], ("through var_ppo_head's g_head", k, e, bound[k])
    # equal inputs, equal bits
    buf2 = Buffers(ctx, kind, n, M)
    assert call(ctx, kind, t, clipped, n, M, buf2) == 0
    again = results(buf2, kind)
    for k in got:
        assert np.array_equal(bits(got[k]), bits(again[k])), k


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("kind,n", HEADS)
@pytest.mark.parametrize("M", SMALL_M)
def test_head_linear_against_float64_and_var_ppo_head(ctx, kind, n, M, clipped):
    check_case(ctx, kind, n, M, clipped)


def test_head_linear_where_the_grid_stride_wraps(ctx):
    check_case(ctx, 0, 4, M_WRAP, True)


def test_head_linear_wrapped_categorical_equals_var_ppo_head(ctx):
    """The widest head past the wrap: bits against var_ppo_head and a second run (the float64 bounds are taken at kind 0)."""
    kind, n, M = 1, 16, M_WRAP
    d, _ = hl.inputs(kind, M, n, 2)
    t = {k: dev(v) for k, v in d.items()}
    buf, buf2 = Buffers(ctx, kind, n, M), Buffers(ctx, kind, n, M)
    assert call(ctx, kind, t, True, n, M, buf) == 0 and call(ctx, kind, t, True, n, M, buf2) == 0
    assert buf.guards_intact() and buf2.guards_intact()
    got, again = results(buf, kind), results(buf2, kind)
    for k in got:
        assert np.array_equal(bits(got[k]), bits(again[k])), k
    out, _, g_value, _ = plain_head(ctx, kind, t, buf.view["head"].view(M, n), True, n, M)
    assert np.array_equal(bits(host(out)), bits(got["out"])) and np.array_equal(bits(host(g_value)), bits(got["g_value"]))


@pytest.mark.parametrize("kind,n,M", [(0, 2, 300), (1, 8, 257)])
def test_a_graph_replay_on_fresh_inputs_equals_eager(ctx, kind, n, M):
    d1, _ = hl.inputs(kind, M, n, 11)
    d2, _ = hl.inputs(kind, M, n, 12)
    static = {k: dev(v) for k, v in d1.items()}
    buf = Buffers(ctx, kind, n, M)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        with torch.cuda.graph(g, stream=side):
            assert call(ctx, kind, static, True, n, M, buf, stream=ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
    torch.cuda.current_stream().wait_stream(side)
    for k, v in d2.items():
        if v is not None:
            static[k].copy_(dev(v))
    g.replay()
    replayed = results(buf, kind)
    assert buf.guards_intact()
    eager = Buffers(ctx, kind, n, M)
    assert call(ctx, kind, {k: dev(v) for k, v in d2.items()}, True, n, M, eager) == 0
    for k, a in results(eager, kind).items():
        assert np.array_equal(bits(a), bits(replayed[k])), k


def test_the_cursor_form_writes_its_statistics_row_and_advances_both_words(ctx):
    kind, n, M, rows = 1, 8, 300, 3
    d, _ = hl.inputs(kind, M, n, 21)
    t = {k: dev(v) for k, v in d.items()}
    buf = Buffers(ctx, kind, n, M)
    stats = torch.full((rows + 2, 3), SENT, device="cuda")       # (a guard row on both sides)
    cursor = torch.tensor([5, 1], dtype=torch.int32, device="cuda")
    assert call(ctx, kind, t, True, n, M, buf, stats=stats[1:], n_stats=rows, cursor=cursor, n_env=4) == 0
    out, s = host(buf.view["out"]), host(stats)
    assert np.array_equal(bits(s[2]), bits(out[:3])) and (np.delete(s, 2, 0) == SENT).all()
    assert host(cursor).tolist() == [9, 2]
    plain = Buffers(ctx, kind, n, M)
    assert call(ctx, kind, t, True, n, M, plain) == 0            # the cursor form changes nothing else
    for k, a in results(plain, kind).items():
        assert np.array_equal(bits(a), bits(host(buf.view[k]))), k
    for row in (rows, -1):                                       # a row outside the table: the words advance, stats stay
        stats.fill_(SENT)
        cursor.copy_(torch.tensor([0, row], dtype=torch.int32))
        assert call(ctx, kind, t, True, n, M, buf, stats=stats[1:], n_stats=rows, cursor=cursor, n_env=4) == 0
        assert (host(stats) == SENT).all() and host(cursor).tolist() == [4, row + 1]


def test_head_linear_refuses_bad_arguments_before_any_launch(ctx, var_amd):
    kind, n, M = 0, 2, 300
    d, _ = hl.inputs(kind, M, n, 31)
    t = {k: dev(v) for k, v in d.items()}
    buf = Buffers(ctx, kind, n, M)
    stats, cursor = torch.full((2, 3), SENT, device="cuda"), torch.tensor([0, 0], dtype=torch.int32, device="cuda")
    off = lambda x, nbytes: ctypes.c_void_p(x.data_ptr() + nbytes)                      # noqa: E731
    cases = {"kind 2": dict(kind=2), "M 0": dict(M=0), "n 0": dict(n=0), "n 5 Gaussian": dict(n=5), "clip < 0": dict(clip=-0.1),
             "clip NaN": dict(clip=float("nan")), "short workspace": dict(ws_bytes=buf.ws_bytes - 4),
             "misaligned workspace": dict(workspace=off(buf.full["workspace"], 4)),
             "misaligned features": dict(features=off(t["features"], 4)), "misaligned g_features": dict(g_features=off(buf.full["g_features"], 4)),
             "g_features overlaps features": dict(g_features=t["features"]), "head overlaps value": dict(head=t["value"]),
             "g_W overlaps W": dict(g_W=t["W"]), "g_b overlaps g_W": dict(g_b=off(buf.view["g_W"], 16)),
             "out overlaps the workspace": dict(out=buf.view["workspace"]), "g_value overlaps head": dict(g_value=buf.view["head"])}
    for name in ("features", "W", "b", "logstd", "value", "action", "old_logp", "adv", "returns", "value_preds", "head", "out", "g_features",
                 "g_W", "g_b", "g_value", "g_logstd", "workspace"):
        cases["NULL " + name] = {name: None}
    for name, over in cases.items():
        rcode = call(ctx, kind, t, True, n, M, buf, over=over)
        assert rcode == -1, name
        with pytest.raises(var_amd.VarHipError):
            ctx.check(rcode, "var_ppo_head_linear")
    assert call(ctx, 1, t, True, 17, M, buf) == -1               # n 17 Categorical
    assert call(ctx, kind, t, True, n, M, buf, stats=stats, n_stats=2) == -1            # stats without a cursor
    assert call(ctx, kind, t, True, n, M, buf, cursor=cursor) == -1                     # a cursor without stats
    assert call(ctx, kind, t, True, n, M, buf, stats=stats, n_stats=0, cursor=cursor) == -1
    assert call(ctx, kind, t, True, n, M, buf, stats=stats, n_stats=2, cursor=cursor, n_env=-1) == -1
    assert call(ctx, kind, t, True, n, M, buf, stats=buf.view["g_features"], n_stats=2, cursor=cursor) == -1     # stats in an output
    assert ctx.lib.var_ppo_head_linear_workspace_bytes(0, 5, M) == -1 and ctx.lib.var_ppo_head_linear_workspace_bytes(1, 8, 0) == -1
    assert buf.untouched() and (host(stats) == SENT).all() and host(cursor).tolist() == [0, 0]
    for k, v in d.items():
        if v is not None:
            assert np.array_equal(host(t[k]), v), k
    assert call(ctx, kind, t, True, n, M, buf, over=dict(value_preds=None)) == -1
    assert call(ctx, kind, t, False, n, M, buf, over=dict(value_preds=None)) == 0                  # (unclipped: value_preds may be NULL)
    assert buf.guards_intact()


def test_ppo_head_linear_autograd_equals_the_c_entry(var_amd, ctx):
    """var_amd.ppo_head_linear: the returns and, scaled by the incoming gradient, the five gradients of the call."""
    for kind, n, M in ((0, 2, 37), (1, 8, 300)):
        d, _ = hl.inputs(kind, M, n, 41)
        t = {k: dev(v) for k, v in d.items()}
        buf = Buffers(ctx, kind, n, M)
        assert call(ctx, kind, t, True, n, M, buf) == 0
        leaves = {k: t[k].clone().requires_grad_() for k in ("features", "W", "b", "value")}
        logstd = t["logstd"].clone().reshape(n, 1).requires_grad_() if kind == 0 else None
        res = var_amd.ppo_head_linear(leaves["features"], leaves["W"], leaves["b"], logstd, leaves["value"], t["action"], t["old_logp"],
                                      t["adv"], t["returns"], t["value_preds"], kind=kind, clip_param=rc.CLIP,
                                      value_loss_coef=rc.VCOEF, entropy_coef=rc.ECOEF)
        out = host(buf.view["out"])
        assert np.array_equal(bits(host(torch.stack(res))), bits(out[[3, 0, 1, 2]]))
        assert res[0].requires_grad and not any(r.requires_grad for r in res[1:])
        (res[0] * 3.0).backward()
        for k, name in (("features", "g_features"), ("W", "g_W"), ("b", "g_b"), ("value", "g_value")):
            assert leaves[k].grad.shape == leaves[k].shape
            assert np.array_equal(bits(host(leaves[k].grad).reshape(-1)), bits(host(buf.view[name] * 3.0))), k
        if kind == 0:
            assert logstd.grad.shape == (n, 1)
            assert np.array_equal(bits(host(logstd.grad).reshape(-1)), bits(host(buf.view["g_logstd"] * 3.0)))
    with pytest.raises(var_amd.VarHipError):
        var_amd.ppo_head_linear(*(torch.zeros(1) for _ in range(10)), kind=0, clip_param=0.2, value_loss_coef=0.5, entropy_coef=0.01)


# ---- var_rollout_move_cursor ---------------------------------------------------------------------------------------------------
def move_tables(segs):
    from var_amd._lib import MoveSeg
    return (MoveSeg * max(len(segs), 1))(*[MoveSeg(*s) for s in segs]), len(segs)


def move_cursor(ctx, segs, ind, n_ind, cursor, n_env, n_src):
    table, k = move_tables(segs)
    return ctx.lib.var_rollout_move_cursor(ctx.handle, None, table, k, p(ind), n_ind, p(cursor), n_env, n_src)


def move(ctx, segs, ind, n_env, n_src):
    table, k = move_tables(segs)
    return ctx.lib.var_rollout_move(ctx.handle, None, table, k, ind, n_env, n_src)


@pytest.mark.parametrize("row_bytes", [4, 12, 16, 27648])
def test_move_cursor_equals_move_at_the_offset_the_word_selects(ctx, row_bytes):
    T, N, nb, n_ind = 3, 5, 2, 10                                # two epochs' permutations behind ind_base
    g = torch.Generator().manual_seed(row_bytes)
    src = torch.randint(0, 256, (T * N * row_bytes,), dtype=torch.uint8, generator=g).cuda()
    hid = torch.randint(0, 256, (N * 16,), dtype=torch.uint8, generator=g).cuda()
    ind = torch.cat([torch.randperm(N, generator=g), torch.randperm(N, generator=g)]).to(torch.int32).cuda()
    size = T * nb * row_bytes
    outs = [torch.full((size + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    houts = [torch.full((nb * 16 + 64,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(2)]
    segs = [[(src.data_ptr(), o.data_ptr() + 16, row_bytes, T, N * row_bytes, nb * row_bytes, row_bytes, row_bytes),
             (hid.data_ptr(), h.data_ptr() + 16, 16, 1, 0, 0, 16, 16)] for o, h in zip(outs, houts)]
    cursor = torch.zeros(2, dtype=torch.int32, device="cuda")
    for k in (0, 3, n_ind - nb):
        for o in outs + houts:
            o.fill_(0xA5)
        cursor.copy_(torch.tensor([k, 7], dtype=torch.int32))
        assert move_cursor(ctx, segs[0], ind, n_ind, cursor, nb, N) == 0
        assert move(ctx, segs[1], ctypes.c_void_p(ind.data_ptr() + 4 * k), nb, N) == 0
        torch.cuda.synchronize()
        assert torch.equal(outs[0], outs[1]) and torch.equal(houts[0], houts[1]), k
        want = src.view(T, N, row_bytes)[:, ind[k:k + nb].long()].reshape(-1)
        assert torch.equal(outs[0][16:16 + size], want) and (outs[0][:16] == 0xA5).all() and (outs[0][16 + size:] == 0xA5).all()
        assert host(cursor).tolist() == [k, 7]                   # the gather reads the word, it does not move it
    for k in (n_ind - nb + 1, -1):                               # the list would leave ind_base[0 .. n_ind): nothing is written
        for o in outs + houts:
            o.fill_(0xA5)
        cursor.copy_(torch.tensor([k, 0], dtype=torch.int32))
        assert move_cursor(ctx, segs[0], ind, n_ind, cursor, nb, N) == 0
        torch.cuda.synchronize()
        assert (outs[0] == 0xA5).all() and (houts[0] == 0xA5).all(), k


def test_move_cursor_refuses_what_move_refuses_and_its_own(ctx, var_amd):
    a = torch.arange(64, dtype=torch.float32, device="cuda")
    b = torch.full((64,), SENT, device="cuda")
    ind = torch.tensor([1, 0, 0, 1], dtype=torch.int32, device="cuda")
    cursor = torch.zeros(2, dtype=torch.int32, device="cuda")
    ok = (a.data_ptr(), b.data_ptr(), 16, 2, 32, 32, 16, 16)
    cases = {
        "no segments": ([], 2, 2), "17 segments": ([ok] * 17, 2, 2), "row_bytes 0": ([(ok[0], ok[1], 0) + ok[3:]], 2, 2),
        "n_t 0": ([ok[:3] + (0,) + ok[4:]], 2, 2), "negative stride": ([ok[:4] + (-32,) + ok[5:]], 2, 2),
        "src NULL": ([(None,) + ok[1:]], 2, 2), "n_env 0": ([ok], 0, 2), "n_src_env 0": ([ok], 2, 0),
        "dst rows overlap": ([ok[:7] + (8,)], 2, 2), "dst steps overlap": ([ok[:5] + (16,) + ok[6:]], 2, 2),
        "dst overlaps src": ([(a.data_ptr(), a.data_ptr() + 16) + ok[2:]], 2, 2),
        "dst overlaps another dst": ([ok, (a.data_ptr(), b.data_ptr() + 32) + ok[2:]], 2, 2),
    }
    for name, (segs, n_env, n_src) in cases.items():
        rcode = move_cursor(ctx, segs, ind, 4, cursor, n_env, n_src)
        assert rcode == -1, name
        with pytest.raises(var_amd.VarHipError):
            ctx.check(rcode, "var_rollout_move_cursor")
        assert move(ctx, segs, p(ind), n_env, n_src) == -1, name                        # var_rollout_move refuses the same
    assert move_cursor(ctx, [ok], None, 4, cursor, 2, 2) == -1
    assert move_cursor(ctx, [ok], ind, 4, None, 2, 2) == -1
    assert move_cursor(ctx, [ok], ind, 0, cursor, 2, 2) == -1
    assert move_cursor(ctx, [ok], ind, 1, cursor, 2, 2) == -1                            # n_env > n_ind
    word = torch.zeros(64, dtype=torch.int32, device="cuda")
    assert move_cursor(ctx, [(a.data_ptr(), word.data_ptr()) + ok[2:]], ind, 4, word[4:], 2, 2) == -1     # dst holds the cursor
    assert move_cursor(ctx, [(a.data_ptr(), word.data_ptr()) + ok[2:]], word[8:], 4, cursor, 2, 2) == -1  # dst holds the list
    torch.cuda.synchronize()
    assert (b == SENT).all() and (word == 0).all() and torch.equal(a, torch.arange(64, dtype=torch.float32, device="cuda"))
    assert move_cursor(ctx, [ok], ind, 4, cursor, 2, 2) == 0
    torch.cuda.synchronize()
    assert torch.equal(b[4:8], a[0:4]) and torch.equal(b[0:4], a[4:8]) and (b[16:] == SENT).all()

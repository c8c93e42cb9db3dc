"""GPU checks of the device clip table: var_ithor_reward_embed, var_ithor_reward_step_ids, var_reward_dots_ids,
IntrinsicReward.build_clip_table / capture(batch, clip_table=...) / step_ids and CollectStep(..., clip_table=...).

Bounds.  One: the embedded clips against the CPU checker at ATOL_CHECKER = 1e-4, the bound tests/test_gpu_ithor_reward.py
holds goal_feat to on the same kernels.  Everything else is bit for bit: a clip's embedding does not depend on the clips that
share its pass (no kernel of the sound branch mixes clips), so var_ithor_reward_embed's rows are the rows the existing entries
write; the id step gathers those rows and forms the dots of tests/clip_table_cpu.py (pinned to IntrinsicReward.reward by
tests/test_clip_table_host.py; products and adds are IEEE float32 operations, the library is built without contraction);
replays against eager calls; CollectStep with a table against the feature-array CollectStep fed the same clips' features."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import _ithor_reward_inputs as rin
from tests import clip_table_cpu as ct
from tests import sound_sound_cpu as ss
from tests import test_gpu_sound_sound as sst                    # its helpers and cached models, not its tests

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_PLAN, ERR_STATE = -1, -3, -4
ATOL_CHECKER = 1e-4
NAN = float("nan")
SOUND_SOUND = 1
N_CLIPS = 32                                                     # + the all-zero clip: a 33-row table

cuda, host, p, bits32, bits64, raw, nans, all_nan, stream = (sst.cuda, sst.host, sst.p, sst.bits32, sst.bits64, sst.raw, sst.nans,
                                                             sst.all_nan, sst.stream)


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.set_num_threads(8)
    return m


@pytest.fixture(scope="module")
def ctx(var_amd):
    from var_amd._lib import Context
    return Context.get(0)


@functools.lru_cache(maxsize=None)
def clips():
    """The reward tests' seeded clips and, last, the all-zero clip the envs send when nothing is heard: (33,1,600,40) on the GPU."""
    return cuda(np.concatenate([rin.spread_sounds(N_CLIPS), np.zeros((1, 1, 600, 40), np.float32)]))


def embed(c, flat, mfcc, n, out):
    return c.lib.var_ithor_reward_embed(c.handle, stream(), p(flat), p(mfcc), n, p(out))


@functools.lru_cache(maxsize=None)
def rows_alone():
    """Every clip embedded by a call of its own (n = 1) on a 16-row plan: what every other build must reproduce bit for bit."""
    _, m = sst.ithor_encoder()
    flat, x = m.flat_parameters(), clips()
    out = nans(N_CLIPS + 1, 3)
    with sst.OwnContext(flat, 16, 0) as c:
        for i in range(N_CLIPS + 1):
            assert embed(c, flat, x[i:i + 1], 1, out[i:i + 1]) == 0, c.lib.var_last_error(c.handle)
        torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())
    return out


# ---- var_ithor_reward_embed -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan,n", [(16, 1), (16, 15), (16, 16), (16, 17), (16, 33), (8, 33)])
def test_embed_rows_do_not_depend_on_their_pass(var_amd, plan, n):
    """The pass edges of a 16-row plan: one clip, one short of a pass, a full pass, a last pass of ONE clip behind one and
    behind two full passes (the all-zero clip, at n = 33); and an 8-row plan, whose passes have 8 clips."""
    _, m = sst.ithor_encoder()
    flat, x, want = m.flat_parameters(), clips(), rows_alone()
    first = N_CLIPS + 1 - n if n < 16 else 0                     # (n = 1: the all-zero clip itself)
    out = nans(n + 1, 3)
    with sst.OwnContext(flat, plan, 0) as c:
        assert embed(c, flat, x[first:], n, out) == 0, c.lib.var_last_error(c.handle)
        torch.cuda.synchronize()
    assert torch.equal(out[:n], want[first:first + n]), f"plan {plan}, n = {n}: a row differs from its n = 1 build"
    assert all_nan(out[n:])                                      # nothing behind the n rows


def test_embed_equals_the_existing_entries_and_the_checker(var_amd):
    """cur_feat of var_ithor_reward_step_ex at B = 1 and 8 (the merged pass: the clips behind 1 and 8 goal clips), goal_feat of
    var_ithor_reward_step at B = 16, and the CPU checker."""
    ref, m = sst.ithor_encoder()
    flat, x, want = m.flat_parameters(), clips(), rows_alone()
    with sst.OwnContext(flat, 16, SOUND_SOUND) as c:
        for B, at in ((1, N_CLIPS), (1, 3), (8, 0), (8, N_CLIPS - 7)):
            img = cuda(rin.spread_images(B))
            o = sst.ex_outs(B)
            assert sst.step_ex(c, flat, img, x[5:5 + B], x[at:at + B], B, **o) == 0, c.lib.var_last_error(c.handle)
            torch.cuda.synchronize()
            assert torch.equal(o["cur_feat"], want[at:at + B]), f"cur_feat at B = {B}, clips {at}.."
            assert torch.equal(o["goal_feat"], want[5:5 + B])
        img, o = cuda(rin.spread_images(16)), [nans(16, 3), nans(16, 3), nans(16)]
        assert sst.step(c, flat, img, x[N_CLIPS - 15:], 16, *o) == 0
        torch.cuda.synchronize()
        assert torch.equal(o[1], want[N_CLIPS - 15:])
    some = [0, 1, 2, 3, 4, 5, 6, 7, N_CLIPS]
    checker = rin.checker_goal_feat(ref, host(x)[some])
    err = np.abs(host(want)[some] - checker).max()
    print(f"var_ithor_reward_embed vs checker: {err:.2e}")
    assert err <= ATOL_CHECKER


def test_embed_refusals_launch_nothing(var_amd):
    from var_amd._lib import Context
    _, m = sst.ithor_encoder()
    flat, x = m.flat_parameters(), clips()
    out = nans(4, 3)
    c = Context(0)
    try:
        assert embed(c, flat, x, 4, out) == ERR_PLAN
        assert c.lib.var_ithor_reward_plan(c.handle, 4, 96) == 0
        assert embed(c, flat, x, 4, out) == ERR_STATE and b"pack" in c.lib.var_last_error(c.handle)
        assert c.lib.var_ithor_reward_pack(c.handle, stream(), p(flat)) == 0
        assert embed(c, flat.clone(), x, 4, out) == ERR_STATE
        assert embed(c, flat, None, 4, out) == ERR_ARG and embed(c, flat, x, 4, None) == ERR_ARG and embed(c, flat, x, 0, out) == ERR_ARG
        assert embed(c, None, x, 4, out) == ERR_ARG
        assert all_nan(out)
        assert embed(c, flat, x, 4, out) == 0                    # a 4-row plan: passes of 4
        torch.cuda.synchronize()
        assert torch.equal(out, rows_alone()[:4])
    finally:
        torch.cuda.synchronize()
        c.lib.var_destroy(c.handle)
        c.handle = None


# ---- var_ithor_reward_step_ids ----------------------------------------------------------------------------------------------
def step_ids(c, flat, image, table, goal_ids, cur_ids, B, image_feat, goal_feat, cur_feat, reward, reward_img, reward_snd, rows=None):
    return c.lib.var_ithor_reward_step_ids(c.handle, stream(), p(flat), p(image), 1, image.stride(0), p(table),
                                           table.shape[0] if rows is None else rows, p(goal_ids), p(cur_ids), B, p(image_feat),
                                           p(goal_feat), p(cur_feat), p(reward), p(reward_img), p(reward_snd))


def ids_case(B):
    """(goal ids of a first step: all valid; goal ids of a second: a mix with -1; current ids of both, `silent` among them)."""
    rng = np.random.default_rng(900 + B)
    g1 = rng.integers(0, N_CLIPS + 1, B).astype(np.int32)
    g2 = rng.integers(0, N_CLIPS + 1, B).astype(np.int32)
    g2[rng.random(B) < 0.5] = -1
    g2[0] = -1
    if B > 1:
        g2[1] = (g1[1] + 1) % N_CLIPS
    c1, c2 = (rng.integers(0, N_CLIPS + 1, B).astype(np.int32) for _ in range(2))
    c1[B // 2], c2[0] = N_CLIPS, N_CLIPS
    return g1, g2, c1, c2


def i32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).cuda()


@pytest.mark.parametrize("B", [1, 8, 9, 63, 64])
def test_step_ids(var_amd, B):
    """B = 8: the last batch whose feature path is the merged pass; 9: one above; 64: the tail's row limit, 63 one short of it.
    Two steps: every env gets a goal, then a mix of new goals and -1.  Every output NaN before."""
    _, m = sst.ithor_encoder()
    flat, x, table = m.flat_parameters(), clips(), rows_alone()
    tab = host(table)
    g1, g2, c1, c2 = ids_case(B)
    imgs = [cuda(rin.spread_images(B)), cuda(rin.spread_images(B, 31))]
    with sst.OwnContext(flat, B, SOUND_SOUND) as c:
        o = sst.ex_outs(B)
        cached, held = np.full((B, 3), NAN, np.float32), None    # goal_feat before the step; the clip every env holds as its goal
        for image, gid, cid in ((imgs[0], g1, c1), (imgs[1], g2, c2)):
            held = gid if held is None else np.where(gid >= 0, gid, held)
            for k in ("image_feat", "cur_feat", "reward", "reward_img", "reward_snd"):
                o[k].fill_(NAN)
            assert step_ids(c, flat, image, table, i32(gid), i32(cid), B, **o) == 0, c.lib.var_last_error(c.handle)
            got = {k: host(v) for k, v in o.items()}
            goal = np.where((gid >= 0)[:, None], tab[np.maximum(gid, 0)], cached)
            assert np.array_equal(bits32(got["goal_feat"]), bits32(goal)), "-1 rows keep goal_feat's bits, the others take the table's"
            assert np.array_equal(bits32(got["cur_feat"]), bits32(tab[cid]))
            # the image rows: what the existing entry writes on an image-only step
            i_ref, g_ref, w_ref = nans(B, 3), cuda(goal), nans(B)
            assert sst.step(c, flat, image, None, B, i_ref, g_ref, w_ref) == 0
            assert np.array_equal(bits32(got["image_feat"]), bits32(host(i_ref)))
            assert np.array_equal(bits32(got["reward_img"]), bits32(host(w_ref)))
            want = ct.step_ids(got["image_feat"], tab, gid, cid, cached)
            for k, w in (("reward", "out"), ("reward_img", "out_img"), ("reward_snd", "out_snd")):
                assert np.array_equal(bits32(got[k]), bits32(want[w])), k
            assert np.isfinite(got["reward"]).all() and np.abs(got["reward_snd"]).max() > 0
            if B <= 8:                                           # the feature path on the same clips, the whole goal batch re-sent
                e = sst.ex_outs(B)
                assert sst.step_ex(c, flat, image, x[torch.from_numpy(held).long().cuda()].contiguous(),
                                   x[torch.from_numpy(cid).long().cuda()].contiguous(), B, **e) == 0
                torch.cuda.synchronize()
                for k in e:
                    assert torch.equal(e[k], o[k]), f"{k} is not var_ithor_reward_step_ex's on the same clips"
            only = nans(B)                                       # the two optional outputs left out
            g_again = cuda(cached)
            assert step_ids(c, flat, image, table, i32(gid), i32(cid), B, o["image_feat"], g_again, o["cur_feat"], only, None, None) == 0
            assert np.array_equal(bits32(host(only)), bits32(got["reward"])) and np.array_equal(bits32(host(g_again)), bits32(goal))
            cached = goal


@pytest.mark.parametrize("B", [8, 64])
def test_step_ids_without_current_ids_is_the_image_only_step(var_amd, B):
    """cur_ids = NULL: var_ithor_reward_step's bits on an image-only step (goal_ids NULL = every row keeps its goal), and with
    goal ids the gathered goal; cur_feat and the two optional outputs stay as they were.  A plan without the sound-sound bit."""
    _, m = sst.ithor_encoder()
    flat, table = m.flat_parameters(), rows_alone()
    g1 = ids_case(B)[0]
    img = cuda(rin.spread_images(B, 31))
    with sst.OwnContext(flat, B, 0) as c:
        o = sst.ex_outs(B)
        assert step_ids(c, flat, img, table, i32(g1), None, B, **o) == 0, c.lib.var_last_error(c.handle)
        torch.cuda.synchronize()
        assert torch.equal(o["goal_feat"], table[torch.from_numpy(g1).long().cuda()])
        want = [nans(B, 3), o["goal_feat"].clone(), nans(B)]
        assert sst.step(c, flat, img, None, B, *want) == 0
        torch.cuda.synchronize()
        assert torch.equal(o["image_feat"], want[0]) and torch.equal(o["reward"], want[2]) and torch.equal(o["goal_feat"], want[1])
        assert all_nan(o["cur_feat"], o["reward_img"], o["reward_snd"])
        o["image_feat"].fill_(NAN), o["reward"].fill_(NAN)
        assert step_ids(c, flat, img, table, None, None, B, **o) == 0
        torch.cuda.synchronize()
        assert torch.equal(o["image_feat"], want[0]) and torch.equal(o["reward"], want[2]) and torch.equal(o["goal_feat"], want[1])


@pytest.mark.parametrize("B", [8, 64])
def test_step_ids_one_bad_id_is_one_nan_row(var_amd, B):
    _, m = sst.ithor_encoder()
    flat, table = m.flat_parameters(), rows_alone()
    g1, g2, c1, c2 = ids_case(B)
    img = cuda(rin.spread_images(B))
    with sst.OwnContext(flat, B, 0) as c:
        good = sst.ex_outs(B)
        assert step_ids(c, flat, img, table, i32(g1), i32(c1), B, **good) == 0
        base = {k: host(v) for k, v in good.items()}
        row = B - 3
        for gbad, cbad in ((N_CLIPS + 1, None), (-2, None), (None, -1), (None, N_CLIPS + 1), (2 ** 31 - 1, None), (None, -2 ** 31)):
            gid, cid = g2.copy(), c2.copy()
            if gbad is not None:
                gid[row] = gbad
            if cbad is not None:
                cid[row] = cbad
            o = {k: cuda(v) for k, v in base.items()}
            w = {k: cuda(v) for k, v in base.items()}
            gid_ok, cid_ok = g2.copy(), c2.copy()
            assert step_ids(c, flat, img, table, i32(gid_ok), i32(cid_ok), B, **w) == 0
            assert step_ids(c, flat, img, table, i32(gid), i32(cid), B, **o) == 0
            got, want = {k: host(v) for k, v in o.items()}, {k: host(v) for k, v in w.items()}
            others = np.arange(B) != row
            for k in got:
                assert np.array_equal(bits32(got[k][others]), bits32(want[k][others])), f"{k}: another row changed"
                if k == "goal_feat":
                    assert np.array_equal(bits32(got[k][row]), bits32(base[k][row])), "the bad row's goal_feat was written"
                else:
                    assert np.isnan(got[k][row]).all(), f"{k} of the bad row is not NaN"


def test_step_ids_refusals_launch_nothing(var_amd):
    from var_amd._lib import Context
    _, m = sst.ithor_encoder()
    flat, table = m.flat_parameters(), rows_alone()
    B = 8
    g1, _, c1, _ = ids_case(B)
    g, cu, img = i32(g1), i32(c1), cuda(rin.spread_images(B))
    c = Context(0)
    try:
        o = sst.ex_outs(B)
        assert step_ids(c, flat, img, table, g, cu, B, **o) == ERR_PLAN
        assert c.lib.var_ithor_reward_plan(c.handle, B, 96) == 0
        assert step_ids(c, flat, img, table, g, cu, B, **o) == ERR_STATE and b"pack" in c.lib.var_last_error(c.handle)
        assert c.lib.var_ithor_reward_pack(c.handle, stream(), p(flat)) == 0
        assert step_ids(c, flat.clone(), img, table, g, cu, B, **o) == ERR_STATE
        big, img9 = sst.ex_outs(B + 1), torch.zeros((B + 1, 3, 96, 96), dtype=torch.uint8, device="cuda")
        assert step_ids(c, flat, img9, table, i32(np.zeros(B + 1)), None, B + 1, **big) == ERR_PLAN and all_nan(*big.values())
        assert step_ids(c, flat, img, table, g, cu, 0, **o) == ERR_ARG
        assert step_ids(c, flat, img, table, g, cu, B, **o, rows=0) == ERR_ARG
        assert b"table" in c.lib.var_last_error(c.handle)
        assert c.lib.var_ithor_reward_step_ids(c.handle, stream(), p(flat), p(img), 1, img.stride(0), None, 33, p(g), p(cu), B,
                                               *(p(o[k]) for k in ("image_feat", "goal_feat", "cur_feat", "reward", "reward_img",
                                                                   "reward_snd"))) == ERR_ARG
        assert step_ids(c, flat, img, table, g, cu, B, o["image_feat"], o["goal_feat"], None, o["reward"], None, None) == ERR_ARG
        assert step_ids(c, flat, img, table, g, cu, B, None, o["goal_feat"], o["cur_feat"], o["reward"], None, None) == ERR_ARG
        assert c.lib.var_ithor_reward_step_ids(c.handle, stream(), p(flat), p(img), 1, 3 * 96 * 96 - 1, p(table), 33, p(g), p(cu), B,
                                               *(p(o[k]) for k in ("image_feat", "goal_feat", "cur_feat", "reward", "reward_img",
                                                                   "reward_snd"))) == ERR_ARG
        assert all_nan(*o.values())
        assert step_ids(c, flat, img, table, g, cu, B, **o) == 0 and not all_nan(o["reward"])      # a plan without the bit serves
    finally:
        torch.cuda.synchronize()
        c.lib.var_destroy(c.handle)
        c.handle = None


def hip_runtime():
    """The HIP runtime this process already runs on (the one torch loaded), not a second copy."""
    for line in open("/proc/self/maps"):
        if "libamdhip64" in line:
            return ctypes.CDLL(line.split()[-1])
    raise AssertionError("no HIP runtime is loaded")


def test_step_ids_is_seven_kernel_nodes(var_amd):
    """The entry captured on a stream: 7 nodes, all kernels -- the ids are data, so goal steps, image-only steps and staggered
    resets are this one graph."""
    _, m = sst.ithor_encoder()
    flat, table = m.flat_parameters(), rows_alone()
    B = 8
    g1, _, c1, _ = ids_case(B)
    g, cu, img = i32(g1), i32(c1), cuda(rin.spread_images(B))
    rt = hip_runtime()
    vp = ctypes.c_void_p
    rt.hipStreamBeginCapture.argtypes, rt.hipStreamEndCapture.argtypes = [vp, ctypes.c_int], [vp, ctypes.POINTER(vp)]
    rt.hipGraphGetNodes.argtypes = [vp, ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_size_t)]
    rt.hipGraphNodeGetType.argtypes, rt.hipGraphDestroy.argtypes = [vp, ctypes.POINTER(ctypes.c_int)], [vp]
    with sst.OwnContext(flat, B, 0) as c:
        o = sst.ex_outs(B)
        for cur in (cu, None):
            assert step_ids(c, flat, img, table, g, cur, B, **o) == 0            # (outside capture first: lazy kernel attributes)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            graph = vp()
            with torch.cuda.stream(side):
                assert rt.hipStreamBeginCapture(side.cuda_stream, 1) == 0        # hipStreamCaptureModeThreadLocal
                rc = step_ids(c, flat, img, table, g, cur, B, **o)
                assert rt.hipStreamEndCapture(side.cuda_stream, ctypes.byref(graph)) == 0 and rc == 0
            n = ctypes.c_size_t(0)
            assert rt.hipGraphGetNodes(graph, None, ctypes.byref(n)) == 0
            nodes = (vp * n.value)()
            assert rt.hipGraphGetNodes(graph, nodes, ctypes.byref(n)) == 0
            kinds = []
            for node in nodes:
                k = ctypes.c_int(-1)
                assert rt.hipGraphNodeGetType(node, ctypes.byref(k)) == 0
                kinds.append(k.value)
            assert rt.hipGraphDestroy(graph) == 0
            assert kinds == [0] * 7, kinds                                       # hipGraphNodeTypeKernel


# ---- var_reward_dots_ids ----------------------------------------------------------------------------------------------------
def dots_ids(c, img, table, goal_ids, cur_ids, goal_feat, cur_feat, rows, dim, out, out_img, out_snd, table_rows=None):
    return c.lib.var_reward_dots_ids(c.handle, stream(), p(img), p(table), table.shape[0] if table_rows is None else table_rows,
                                     p(goal_ids), p(cur_ids), p(goal_feat), p(cur_feat), rows, dim, p(out), p(out_img), p(out_snd))


@pytest.mark.parametrize("dim", [3, 64])
@pytest.mark.parametrize("rows", [1, 255, 256, 257])
def test_reward_dots_ids_equal_the_restatement_bit_for_bit(ctx, rows, dim):
    """rows around the 256-thread block edge; dim 3 (the embeddings) and 64 (the entry's limit); a 33-row table; about a third
    of the goal ids -1, one id of each kind out of range where there is room."""
    rng = np.random.default_rng(7 * dim + rows)
    img, cached, _ = ss.unit_rows(rows, dim, seed=100 * dim + rows)
    table = ct.unit_table(33, dim, seed=5)
    gid, cid = rng.integers(0, 33, rows).astype(np.int32), rng.integers(0, 33, rows).astype(np.int32)
    gid[rng.random(rows) < 1 / 3] = -1
    if rows > 200:
        gid[17], gid[130], cid[64], cid[200] = 33, -2, -1, 2 ** 31 - 1
    d_img, d_tab = cuda(img), cuda(table)
    want = ct.step_ids(img, table, gid, cid, cached)
    assert int(want["bad"].sum()) == (4 if rows > 200 else 0)
    goal, cur, out, a, b = cuda(cached), nans(rows, dim), nans(rows), nans(rows), nans(rows)
    assert dots_ids(ctx, d_img, d_tab, i32(gid), i32(cid), goal, cur, rows, dim, out, a, b) == 0, ctx.lib.var_last_error(ctx.handle)
    for got, k in ((out, "out"), (a, "out_img"), (b, "out_snd"), (goal, "goal_feat"), (cur, "cur_feat")):
        assert np.array_equal(bits32(host(got)), bits32(want[k])), k
    # no current ids: the first dot alone, cur_feat untouched; no goal ids: every row keeps its embedding
    goal, cur, out, a, b = cuda(cached), nans(rows, dim), nans(rows), nans(rows), nans(rows)
    assert dots_ids(ctx, d_img, d_tab, i32(gid), None, goal, None, rows, dim, out, a, b) == 0
    off = ct.step_ids(img, table, gid, None, cached)
    assert np.array_equal(bits32(host(out)), bits32(off["out"])) and np.array_equal(bits32(host(a)), bits32(off["out_img"]))
    ok = ~off["bad"]
    assert not host(b)[ok].any() and np.array_equal(bits32(host(goal)), bits32(off["goal_feat"]))
    only = nans(rows)
    assert dots_ids(ctx, d_img, d_tab, None, i32(np.where(want["bad"], 0, cid)), goal, cur, rows, dim, only, None, None) == 0
    kept = ct.step_ids(img, table, None, np.where(want["bad"], 0, cid), off["goal_feat"])
    assert np.array_equal(bits32(host(only)), bits32(kept["out"])) and np.array_equal(bits32(host(goal)), bits32(off["goal_feat"]))


@pytest.mark.parametrize("rows,dim", [(257, 3), (255, 64)])
def test_reward_dots_ids_with_valid_ids_is_reward_dots_on_gathered_rows(ctx, rows, dim):
    rng = np.random.default_rng(rows)
    img = ss.unit_rows(rows, dim, seed=3)[0]
    table = ct.unit_table(33, dim, seed=5)
    gid, cid = rng.integers(0, 33, rows).astype(np.int32), rng.integers(0, 33, rows).astype(np.int32)
    d_img, d_tab = cuda(img), cuda(table)
    goal, cur, out, a, b = nans(rows, dim), nans(rows, dim), nans(rows), nans(rows), nans(rows)
    assert dots_ids(ctx, d_img, d_tab, i32(gid), i32(cid), goal, cur, rows, dim, out, a, b) == 0
    w_out, w_a, w_b = nans(rows), nans(rows), nans(rows)
    assert sst.dots(ctx, d_img, cuda(table[gid]), cuda(table[cid]), rows, dim, w_out, w_a, w_b) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, w_out) and torch.equal(a, w_a) and torch.equal(b, w_b)
    assert torch.equal(goal, cuda(table[gid])) and torch.equal(cur, cuda(table[cid]))


def test_reward_dots_ids_refuses_bad_arguments_and_writes_nothing(ctx):
    rows, dim = 5, 3
    img, cached, _ = (cuda(a) for a in ss.unit_rows(rows, dim, seed=1))
    table = cuda(ct.unit_table(33, dim, seed=5))
    keep = cached.clone()
    g, cu = i32(np.arange(rows)), i32(np.arange(rows) + 3)
    cur, out, a, b = nans(rows, dim), nans(rows), nans(rows), nans(rows)
    assert dots_ids(ctx, img, table, g, cu, cached, cur, 0, dim, out, a, b) == ERR_ARG
    assert b"var_reward_dots_ids" in ctx.lib.var_last_error(ctx.handle)
    assert dots_ids(ctx, img, table, g, cu, cached, cur, rows, 65, out, a, b) == ERR_ARG
    assert dots_ids(ctx, img, table, g, cu, cached, cur, rows, 0, out, a, b) == ERR_ARG
    assert dots_ids(ctx, None, table, g, cu, cached, cur, rows, dim, out, a, b) == ERR_ARG
    assert dots_ids(ctx, img, table, g, cu, None, cur, rows, dim, out, a, b) == ERR_ARG
    assert dots_ids(ctx, img, table, g, cu, cached, None, rows, dim, out, a, b) == ERR_ARG      # cur_ids without cur_feat
    assert dots_ids(ctx, img, table, g, cu, cached, cur, rows, dim, None, a, b) == ERR_ARG
    assert dots_ids(ctx, img, table, g, cu, cached, cur, rows, dim, out, a, b, table_rows=0) == ERR_ARG
    assert ctx.lib.var_reward_dots_ids(ctx.handle, stream(), p(img), None, 33, p(g), p(cu), p(cached), p(cur), rows, dim, p(out), p(a),
                                       p(b)) == ERR_ARG
    assert all_nan(cur, out, a, b) and torch.equal(cached, keep)
    assert dots_ids(ctx, img, table, g, cu, cached, cur, rows, dim, out, a, b) == 0 and not all_nan(out)


# ---- ClipTable, capture(batch, clip_table=...) ------------------------------------------------------------------------------
def kuka_clips(n, seed):
    return np.random.default_rng(seed).standard_normal((n, 1, 100, 40)).astype(np.float32)


def test_ithor_clip_table_from_features_and_from_pcm(var_amd):
    _, m = sst.ithor_encoder()
    r = var_amd.IntrinsicReward(m)
    t = r.build_clip_table(features=host(clips())[:N_CLIPS])
    assert isinstance(t, var_amd.ClipTable) and (t.rows, t.silent, tuple(t.feat.shape)) == (N_CLIPS, N_CLIPS, (N_CLIPS + 1, 3))
    assert torch.equal(t.feat, rows_alone())                     # row `silent` = the all-zero clip's embedding
    assert torch.equal(r.build_clip_table(features=clips()[:N_CLIPS], chunk=5).feat, t.feat)
    from var_amd.data import synth_clips
    pcm = synth_clips(5, seed=3)
    lens = np.array([16000, 12000, 1, 16000, 8000], np.int32)
    from_pcm = r.build_clip_table(pcm=pcm, lens=lens, chunk=2)
    feats = var_amd.mfcc_psf(cuda(pcm), cuda(lens), out_frames=600)
    assert torch.equal(from_pcm.feat, r.build_clip_table(features=feats).feat)
    assert from_pcm.rows == 5 and bool(torch.isfinite(from_pcm.feat).all())
    with pytest.raises(var_amd.VarHipError):
        r.build_clip_table()
    with pytest.raises(var_amd.VarHipError):
        r.build_clip_table(features=feats, pcm=pcm)
    with pytest.raises(var_amd.VarHipError):
        r.build_clip_table(features=kuka_clips(3, 1))


@pytest.mark.parametrize("hw", [96, 84])
def test_kuka_clip_table_rows_do_not_depend_on_the_chunk(var_amd, ctx, golden_dir, hw):
    """The Kuka sound CNN is one workgroup per clip and its head a per-row product: chunks of 256, 7 and 1 clips give the same
    bits, and they are the bits the forward of a reward step writes for the clip as its goal (B = 8, beside an image) and as
    its current sound."""
    m = sst.kuka_model(golden_dir, hw)
    r = var_amd.IntrinsicReward(m)
    feats = kuka_clips(33, 4)
    t = r.build_clip_table(features=feats)
    assert tuple(t.feat.shape) == (34, 3) and bool(torch.isfinite(t.feat).all())
    for chunk in (7, 1):
        assert torch.equal(r.build_clip_table(features=cuda(feats), chunk=chunk).feat, t.feat), f"chunk {chunk}"
    B, flat = 8, m.flat_parameters()
    img = cuda(np.random.default_rng(1).integers(0, 256, size=(B, 3, hw, hw), dtype=np.uint8))
    feat, pos, neg = nans(B, 3), nans(B, 3), nans(B, 3)
    ctx.ensure_plan(B, hw)
    m.hip_weights(ctx).bind()
    x = cuda(np.concatenate([feats, np.zeros((1, 1, 100, 40), np.float32)]))
    ctx.check(ctx.lib.var_arm_encoder_fwd(ctx.handle, stream(), p(flat), p(img), 1, img.stride(0), p(x[3:11]), p(x[26:34]), B, hw, p(feat),
                                          p(pos), p(neg), None, None, 2), "var_arm_encoder_fwd")
    torch.cuda.synchronize()
    assert torch.equal(pos, t.feat[3:11]) and torch.equal(neg, t.feat[26:34])
    from var_amd.data import synth_clips
    pcm, lens = synth_clips(5, seed=3), np.array([16000, 12000, 1, 16000, 8000], np.int32)
    assert torch.equal(r.build_clip_table(pcm=pcm, lens=lens, chunk=3).feat,
                       r.build_clip_table(features=var_amd.mfcc(cuda(pcm), cuda(lens))).feat)


def replay_case(k, B, rows):
    rng = np.random.default_rng(1000 + k)
    gid = rng.integers(0, rows + 1, B).astype(np.int32)
    if k % 4:
        gid[rng.random(B) < 0.7] = -1
    return gid, rng.integers(0, rows + 1, B).astype(np.int32)


@pytest.mark.parametrize("sound_sound", [True, False])
def test_ithor_capture_with_a_clip_table(var_amd, ctx, sound_sound):
    """Twenty replays with changing ids -- host arrays on even steps, device tensors on odd ones; new goals for all, for some
    and for none -- equal eager calls of the entry."""
    _, m = sst.ithor_encoder()
    B = 8
    r = var_amd.IntrinsicReward(m, sound_sound=sound_sound)
    table = r.build_clip_table(features=clips()[:N_CLIPS])
    assert r.capture(B, clip_table=table) is r and list(r._graphs) == ["ids"]
    flat = m.flat_parameters()
    gen = torch.Generator(device="cuda").manual_seed(78)
    e = sst.ex_outs(B)
    e["goal_feat"].zero_()
    with pytest.raises(var_amd.VarHipError, match="goal"):
        r.step_ids(torch.zeros((B, 3, 96, 96), dtype=torch.uint8, device="cuda"), None, np.zeros(B, np.int32))
    for k in range(20):
        img = torch.randint(0, 256, (B, 3, 96, 96), dtype=torch.uint8, device="cuda", generator=gen)
        gid, cid = replay_case(k, B, table.rows)
        dev = k % 2 == 1
        goal_arg = None if (k % 4 == 3) else (i32(gid) if dev else gid)
        i, g, w = r.step_ids(img, goal_arg, i32(cid) if dev else cid)
        assert step_ids(ctx, flat, img, table.feat, None if goal_arg is None else i32(gid), i32(cid) if sound_sound else None, B,
                        **e) == 0, ctx.lib.var_last_error(ctx.handle)
        torch.cuda.synchronize()
        same = torch.equal(i, e["image_feat"]) and torch.equal(g, e["goal_feat"]) and torch.equal(w, e["reward"])
        if sound_sound:
            same = same and (torch.equal(r.cur_feat, e["cur_feat"]) and torch.equal(r.img_sound_dot, e["reward_img"]) and
                             torch.equal(r.sound_sound_dot, e["reward_snd"]))
        assert same, f"replay {k} differs from the eager call"
        assert bool(torch.isfinite(w).all())
    before = raw(r._img), raw(r._ids), raw(r._reward), raw(r._goal_feat)
    bad = gid.copy()
    bad[2] = table.rows + 1
    with pytest.raises(var_amd.VarHipError, match="ids outside"):
        r.step_ids(img + 1, bad, cid)
    with pytest.raises(var_amd.VarHipError, match="ids outside"):
        r.step_ids(img + 1, np.where(np.arange(B) == 1, -2, gid), cid)
    if sound_sound:
        with pytest.raises(var_amd.VarHipError, match="ids outside"):
            r.step_ids(img + 1, gid, np.where(np.arange(B) == 1, -1, cid))      # -1 is no current id
        with pytest.raises(var_amd.VarHipError, match="current_ids"):
            r.step_ids(img + 1, gid)
    assert all(np.array_equal(a, b) for a, b in zip(before, (raw(r._img), raw(r._ids), raw(r._reward), raw(r._goal_feat))))


@pytest.mark.parametrize("hw", [96, 84])
def test_kuka_capture_with_a_clip_table(var_amd, ctx, golden_dir, hw):
    """Twenty replays equal the eager pair: the image-only forward, then var_reward_dots_ids; and the embeddings are the ones
    the feature-array capture computes from the same clips."""
    B = 8
    m = sst.kuka_model(golden_dir, hw)
    r = var_amd.IntrinsicReward(m, sound_sound=True)
    feats = kuka_clips(12, 9)
    table = r.build_clip_table(features=feats)
    r.capture(B, clip_table=table)
    flat = m.flat_parameters()
    rng = np.random.default_rng(hw)
    goal, cur, out, a, b, feat = nans(B, 3), nans(B, 3), nans(B), nans(B), nans(B), nans(B, 3)
    goal.zero_()
    for k in range(20):
        img = cuda(rng.integers(0, 256, size=(B, 3, hw, hw), dtype=np.uint8))
        gid, cid = replay_case(k, B, table.rows)
        dev = k % 2 == 1
        goal_arg = None if (k % 4 == 3) else (i32(gid) if dev else gid)
        f, g, w = r.step_ids(img, goal_arg, i32(cid) if dev else cid)
        ctx.ensure_plan(B, hw)
        m.hip_weights(ctx).bind()
        ctx.check(ctx.lib.var_arm_encoder_fwd(ctx.handle, stream(), p(flat), p(img), 1, img.stride(0), None, None, B, hw, p(feat), None,
                                              None, None, None, 2), "var_arm_encoder_fwd")
        assert dots_ids(ctx, feat, table.feat, None if goal_arg is None else i32(gid), i32(cid), goal, cur, B, 3, out, a, b) == 0
        torch.cuda.synchronize()
        same = (torch.equal(f, feat) and torch.equal(g, goal) and torch.equal(w, out) and torch.equal(r.cur_feat, cur) and
                torch.equal(r.img_sound_dot, a) and torch.equal(r.sound_sound_dot, b))
        assert same, f"replay {k} differs from the eager calls"
    # against the feature-array capture on the same clips: a goal step for all, then a current-only step
    x = np.concatenate([feats, np.zeros((1, 1, 100, 40), np.float32)])
    old = var_amd.IntrinsicReward(m, sound_sound=True).capture(B)
    gid, cid = replay_case(0, B, table.rows)
    for goal_ids in (gid, None):
        img = cuda(rng.integers(0, 256, size=(B, 3, hw, hw), dtype=np.uint8))
        got = [host(t) for t in r.step_ids(img, goal_ids, cid)] + [host(r.cur_feat), host(r.img_sound_dot), host(r.sound_sound_dot)]
        want = [host(t) for t in old.step(img, None if goal_ids is None else cuda(x[gid]), cuda(x[cid]))]
        want += [host(old.cur_feat), host(old.img_sound_dot), host(old.sound_sound_dot)]
        assert all(np.array_equal(bits32(u), bits32(v)) for u, v in zip(got, want))


def test_a_stale_table_is_refused_and_a_rebuilt_one_differs(var_amd):
    import var_amd as va
    ref = rin.spread_checker()
    m = va.IthorVARPretextNet(sst.cfg96())
    m.load_state_dict(ref.state_dict())
    m = m.to("cuda").eval()
    B = 8
    r = va.IntrinsicReward(m)
    x = clips()[:4]
    table = r.build_clip_table(features=x)
    r.capture(B, clip_table=table)
    img = torch.zeros((B, 3, 96, 96), dtype=torch.uint8, device="cuda")
    r.step_ids(img, np.arange(B) % 5)
    m.load_state_dict(rin.spread_checker(head_seed=6).state_dict())
    with pytest.raises(va.VarHipError, match="build the table again"):
        r.step_ids(img, np.arange(B) % 5)
    with pytest.raises(va.VarHipError, match="build the table again"):
        r.capture(B, clip_table=table)
    with pytest.raises(va.VarHipError, match="build the table again"):
        va.IntrinsicReward(sst.ithor_encoder()[1]).capture(B, clip_table=table)      # another model's table
    again = r.build_clip_table(features=x)
    assert not torch.equal(again.feat, table.feat) and bool(torch.isfinite(again.feat).all())
    r.capture(B, clip_table=again).step_ids(img, np.arange(B) % 5)
    torch.cuda.synchronize()
    assert torch.equal(r._goal_feat, again.feat[torch.arange(B).cuda() % 5])


# ---- CollectStep ------------------------------------------------------------------------------------------------------------
N_ENVS, T_STEPS, N_OBSERVE, POOL = sst.N_ENVS, sst.T_STEPS, sst.N_OBSERVE, 12
DONE_AT = {2: 5, 4: 2}                                           # step -> the env that finishes there; its new goal comes one step later


@functools.lru_cache(maxsize=None)
def collect_inputs(which):
    """A pool of 12 clips; step 0 is envs.reset(), steps 1..6 what the simulator returns.  Env 5 finishes at step 2 and env 2 at
    step 4; each gets a new goal alone at the next step.  `goals[t]`: every env's goal clip during step t."""
    rng = np.random.default_rng(41 if which == "arm" else 42)
    frames = 100 if which == "arm" else 600
    pool = rng.normal(size=(POOL, 1, frames, 40)).astype(np.float32)
    goals = [rng.integers(0, POOL, N_ENVS).astype(np.int32)]
    steps = []
    for t in range(N_OBSERVE + 1):
        d = dict(image=rng.integers(0, 256, size=(N_ENVS, 3, 96, 96), dtype=np.uint8),
                 env_reward=rng.normal(0, 1.5, size=N_ENVS) * (rng.random(N_ENVS) < 0.6), done=np.zeros(N_ENVS, bool),
                 bad=rng.random(N_ENVS) < 0.15, current_ids=rng.integers(0, POOL + 1, N_ENVS).astype(np.int32))
        d["current_ids"][t % N_ENVS] = POOL                      # nothing is heard there
        d["extras"] = ({'robot_pose': rng.normal(size=(N_ENVS, 2)).astype(np.float32)} if which == "arm" else
                       {'occupancy': ((rng.random((N_ENVS, 1, 9, 9)) < 0.3) * 255).astype(np.uint8)})
        d["goal_ids"] = None
        if t in DONE_AT:
            d["done"][DONE_AT[t]] = True
        if t - 1 in DONE_AT:
            env = DONE_AT[t - 1]
            g = goals[-1].copy()
            g[env] = (g[env] + 1 + rng.integers(0, POOL - 1)) % POOL
            goals.append(g)
            d["goal_ids"] = np.where(np.arange(N_ENVS) == env, g, -1).astype(np.int32)
        elif t > 0:
            goals.append(goals[-1])
        steps.append(d)
    return pool, np.concatenate([pool, np.zeros((1, 1, frames, 40), np.float32)]), goals, steps


def collect_leg(var_amd, which, sound_sound, with_table, seed=5):
    enc, pol, space, cfg = sst.models(which)
    pool, x, goals, steps = collect_inputs(which)
    act = pol.capture(N_ENVS, seed=seed)
    ro = sst.storage(var_amd, which, act)
    reward = var_amd.IntrinsicReward(enc, sound_sound=sound_sound)
    if with_table:
        table = reward.build_clip_table(features=pool)
        cs = var_amd.CollectStep(reward, act, ro, clip_table=table)
        assert sorted(cs._graphs) == ["reset", "step"] and cs._small.numel() == (8 + 2 + 2 * 4) * N_ENVS
        cs.reset(steps[0]["image"], steps[0]["extras"], goal_ids=goals[0])
    else:
        cs = var_amd.CollectStep(reward, act, ro)
        cs.reset(steps[0]["image"], steps[0]["extras"], x[goals[0]])
    snaps, dots, refusal = [], [], None
    for t in range(1, N_OBSERVE + 1):
        act(act.obs, act.masks)
        d = steps[t]
        if with_table:
            if t == T_STEPS + 1:                                 # behind the slot wrap: a bad host id
                def everything():
                    s = sst.snapshot(ro)
                    s.update(f64=raw(cs.norm._f64), slot=raw(cs.norm.slot), masks_buf=raw(act.masks), image_buf=raw(act.obs['image']),
                             small=raw(cs._small), dot=raw(cs.dot), goal=raw(act.obs['goal_sound_feat']))
                    return s
                before, step_before = everything(), ro.step
                bad_ids = np.where(np.arange(N_ENVS) == 3, POOL + 1, -1)
                with pytest.raises(var_amd.VarHipError, match="ids outside"):
                    cs.observe(d["image"], d["extras"], d["env_reward"], d["done"], d["bad"], goal_ids=bad_ids, current_ids=d["current_ids"])
                if sound_sound:
                    with pytest.raises(var_amd.VarHipError, match="ids outside"):
                        cs.observe(d["image"], d["extras"], d["env_reward"], d["done"], d["bad"], goal_ids=d["goal_ids"],
                                   current_ids=np.full(N_ENVS, -1))
                    with pytest.raises(var_amd.VarHipError, match="current_ids"):
                        cs.observe(d["image"], d["extras"], d["env_reward"], d["done"], d["bad"], goal_ids=d["goal_ids"])
                after = everything()
                refusal = ro.step == step_before and all(np.array_equal(before[k], after[k]) for k in before)
            dev = t % 2 == 1                                     # host ids on even steps, device tensors on odd ones
            gid = d["goal_ids"] if (d["goal_ids"] is None or not dev) else i32(d["goal_ids"])
            r = cs.observe(d["image"], d["extras"], d["env_reward"], d["done"], d["bad"], goal_ids=gid,
                           current_ids=(i32(d["current_ids"]) if dev else d["current_ids"]) if sound_sound else None)
        else:                                                    # the whole batch's goal re-sent where one env got a new one
            goal = None if d["goal_ids"] is None else x[goals[t]]
            r = cs.observe(d["image"], d["extras"], d["env_reward"], d["done"], d["bad"], goal, x[d["current_ids"]] if sound_sound else None)
        assert r is cs.norm.reward and ro.step == t % T_STEPS
        dots.append((host(cs.dot),) + ((host(cs.dot_img), host(cs.dot_snd), host(cs.cur_feat)) if sound_sound else ()))
        if t % T_STEPS == 0 or t == N_OBSERVE:
            snaps.append(sst.snapshot(ro))
            ro.after_update()
    torch.cuda.synchronize()
    return dict(snaps=snaps, state=cs.norm.state(), step=ro.step, stats=cs.episode_stats(), dots=dots, refusal=refusal)


@pytest.mark.parametrize("sound_sound", [True, False])
@pytest.mark.parametrize("which", ["arm", "ithor"])
def test_collect_step_with_a_clip_table_equals_the_feature_array_step(var_amd, which, sound_sound):
    """N = 8, T = 4, six observes across the slot wrap; two envs finish at different steps and each gets a new goal alone, where
    the feature-array CollectStep needs the whole batch's goal sounds again."""
    _, _, goals, steps = collect_inputs(which)
    assert [t for t, d in enumerate(steps) if d["goal_ids"] is not None] == [3, 5]
    assert all((d["goal_ids"] >= 0).sum() == 1 for d in steps if d["goal_ids"] is not None)
    want = collect_leg(var_amd, which, sound_sound, False)
    got = collect_leg(var_amd, which, sound_sound, True)
    assert len(got["snaps"]) == len(want["snaps"]) == 2 and got["step"] == want["step"] == N_OBSERVE % T_STEPS
    for sa, sb in zip(got["snaps"], want["snaps"]):
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), k
    assert got["state"][:3] == want["state"][:3] and np.array_equal(bits64(got["state"][3]), bits64(want["state"][3]))
    for key in ("running", "last", "finished"):
        assert np.array_equal(bits64(got["stats"][key]), bits64(want["stats"][key])), key
    assert got["stats"]["finished"].sum() == 2
    for a, b in zip(got["dots"], want["dots"]):
        assert len(a) == len(b) and all(np.array_equal(bits32(u), bits32(v)) for u, v in zip(a, b))
    assert got["refusal"] is True, "a step refused for a bad id changed the storage, the normaliser, the buffers or the slot"

"""Host twin of tests/test_gpu_inbatch_dp.py: the multi-rank branch of VARTrainer.capture_inbatch_epoch_steps -- four graphs with
three eager collectives between them, the static cand (M,3) / ccls (M) buffers, allgather(..., out=...), the rank offset lo = rank *
2B in the captured pointers, the classes gathered again on every replay -- on two gloo ranks on the CPU, the library's entries bound
to the oracle (tests/_oracle_ctx.py, tests/test_inbatch_classes_host.py: OracleContextEx).  B_local = 3: 2B = 6, M = 12, so rank 1's
rows start at lo = 6, no multiple of the 4 rows a head workgroup takes.  Three replays over a two-row table (the third wraps), then
load_table with the rows swapped and two more; every replay against ONE process on the global batch in the ranks' candidate order
(_full_batch_reference, at that module's bounds) and against the eager two-rank step_inbatch on the same rows.

Faults planted in inbatch.py on a scratch copy, and the modes in which this module then fails ("all" / the class-aware two):
    self.lo = 0                                    fails / fails      (rank 1 scores and back-propagates rank 0's rows)
    gather() gathers the classes once only          passes / fails    (mode "all" gathers no classes)
    reduce() does nothing                          fails / fails
    mine = gc[:2B] in backward()                   fails / fails"""
import functools

import numpy as np
import pytest
import torch

import var_amd
from tests import inbatch_classes_cpu as ic
from tests._inbatch_dp import ITEMS, NAMES, assert_classes_differ, candidate_classes, init_group, rank_items, report, run_ranks
from tests.test_gpu_dp2 import _tables
from tests.test_inbatch_classes_host import OracleContextEx, _cfg, _features, _full_batch_reference, _pool

B = 3                                                   # per rank
ROWS = (0, 1, 0, 1, 0)                                  # the row of ITEMS each replay steps: 0 1 0(wrap), then swapped: 1 0
SWAP_AT = 3


def _log(tr, name):
    """Put the trainer's collectives into the call record of its oracle library, beside the library's entries."""
    inner, calls = getattr(tr, name), tr.ctx.lib.calls

    def logged(t, *a, **k):
        calls.append((name, tuple(t.shape)))
        return inner(t, *a, **k)
    setattr(tr, name, logged)


def _kw(negatives, gt, sn):
    return {} if negatives == "all" else dict(classes=(gt, sn), negatives=negatives)


def _rank(rank, world, port, negatives):
    init_group(rank, world, port)
    torch.set_num_threads(2)
    torch.manual_seed(5 + rank)                              # different initial weights: the trainer broadcasts rank 0's
    mc, me = var_amd.VARPretextNet(_cfg()), var_amd.VARPretextNet(_cfg())
    me.load_state_dict(mc.state_dict())
    tc = var_amd.VARTrainer(mc, lr=1e-3, _ctx=OracleContextEx())
    te = var_amd.VARTrainer(me, lr=1e-3, _ctx=OracleContextEx())
    pool = _pool(12)
    gt_tab, sn_tab = pool.class_tables()
    table = _tables(pool, world, B, ITEMS)[rank]
    for name in ("allgather", "allreduce_sum"):
        _log(tc, name)
    replay, load_table = tc.capture_inbatch_epoch_steps(pool.images, pool.clips, B, table, tau=0.1, **_kw(negatives, gt_tab, sn_tab))
    cand, lcls, ccls = tc._keep_inbatch[3], tc._keep_inbatch[5], tc._keep_inbatch[6]
    steps = [dict(params=mc.flat_parameters().numpy().copy())]           # (entry 0: where both replicas start)
    for s, row in enumerate(ROWS):
        if s == SWAP_AT:
            load_table(table.flip(0).contiguous())
        for dst, src in ((me.flat_parameters(), mc.flat_parameters()), (te.exp_avg, tc.exp_avg), (te.exp_avg_sq, tc.exp_avg_sq)):
            dst.copy_(src)                                   # the eager step starts where this replay starts
        loss = float(replay().item())
        mine = torch.tensor(rank_items(ITEMS[row], rank, world))
        r = table[row]
        eager = float(te.step_inbatch(pool.images[mine].contiguous(), _features(pool, r[B:2 * B], r[3 * B:4 * B]),
                                      _features(pool, r[2 * B:3 * B], r[4 * B:]), tau=0.1,
                                      **_kw(negatives, gt_tab[mine].contiguous(), sn_tab[mine].contiguous())).item())
        steps.append(dict(loss=loss, eager=eager, gbuf=tc.gbuf.numpy().copy(), eager_gbuf=te.gbuf.numpy().copy(),
                          params=mc.flat_parameters().numpy().copy(), eager_params=me.flat_parameters().numpy().copy(),
                          cand=cand.numpy().copy(), lcls=lcls.numpy().copy(), ccls=ccls.numpy().copy()))
    return steps, list(tc.ctx.lib.calls), tc.step_count


def _worker(rank, world, port, out, negatives):
    report(out, rank, _rank, rank, world, port, negatives)


@functools.lru_cache(maxsize=None)
def _two_ranks(negatives):
    return run_ranks(_worker, (negatives,), wait=600)


def _state_dict(flat):
    sd, o = {}, 0
    for k, s in var_amd.PARAM_SPECS:
        n = int(np.prod(s))
        sd[k] = torch.from_numpy(flat[o:o + n].copy()).view(s)
        o += n
    return sd


def test_the_rows_tell_the_ranks_and_the_steps_apart():
    pool = _pool(12)
    gt_tab, sn_tab = pool.class_tables()
    assert_classes_differ(gt_tab, sn_tab)
    tabs = _tables(pool, 2, B, ITEMS)
    assert all(t.shape == (2, 5 * B) for t in tabs) and not torch.equal(tabs[0], tabs[1])
    # rank 1's anchors of row 0 find their classes among rank 0's candidates: a mask that stops at the rank's own rows shows
    z0 = candidate_classes(gt_tab, sn_tab, rank_items(ITEMS[0], 0), 1).tolist()
    assert sum(int(y) in z0 for y in gt_tab[rank_items(ITEMS[0], 1)].tolist()) >= 2


@pytest.mark.parametrize("negatives", NAMES)
def test_captured_four_graph_step_on_two_ranks(negatives):
    mode = ic.MODES[negatives]
    got = _two_ranks(negatives)
    pool = _pool(12)
    gt_tab, sn_tab = pool.class_tables()
    assert np.array_equal(got[0][0][0]["params"], got[1][0][0]["params"])            # the broadcast
    worst = dict(loss=0.0, arena=0.0, eager_params=0.0, blind=0.0)
    for s, row in enumerate(ROWS):
        items = ITEMS[row]
        i = torch.tensor(items)
        sd = _state_dict(got[0][0][s]["params"])
        snd = torch.stack([_features(pool, pool.clip_tab[k, i], pool.len_tab[k, i]) for k in (0, 1)])
        gt, sn = gt_tab[i], sn_tab[i]
        loss, G = _full_batch_reference(sd, pool.images[i], snd, gt, sn, 2, mode)
        blind, _ = _full_batch_reference(sd, pool.images[i], snd, gt, sn, 2, ic.ALL)
        worst["blind"] = max(worst["blind"], abs(loss - blind))
        zs = candidate_classes(gt_tab, sn_tab, items).numpy()
        for rank in range(2):
            st = got[rank][0][s + 1]
            assert abs(st["loss"] - loss) < 2e-6 and abs(st["gbuf"][-1] - loss) < 2e-6, (s, rank, st["loss"], loss)
            d = float(np.max(np.abs(st["gbuf"][:-1] - G)))
            assert d < 1e-5 * max(1.0, np.max(np.abs(G))), (s, rank, d)
            worst["loss"], worst["arena"] = max(worst["loss"], abs(st["loss"] - loss)), max(worst["arena"], d)
            # against the eager two-rank step from the same parameters and moments on the same rows: the same oracle entries
            # on the same bits in the same order, so the same loss and arena; the Adam entries differ in the learning rate alone
            # (f32(1e-3) from the device scalar against the double 1e-3), a relative 2^-24 of an update of a few lr at the most
            # (< 1e-9), and then one rounding of the parameter
            assert st["loss"] == st["eager"] and np.array_equal(st["gbuf"], st["eager_gbuf"]), (s, rank, st["loss"], st["eager"])
            dp = np.abs(st["params"] - st["eager_params"])
            assert (dp <= np.spacing(np.abs(st["params"])) + 1e-9).all(), (s, rank, float(dp.max()))
            worst["eager_params"] = max(worst["eager_params"], float(dp.max()))
            if mode:                                                                  # the static class buffers, on every replay
                assert np.array_equal(st["lcls"], zs[6 * rank:6 * rank + 6]) and np.array_equal(st["ccls"], zs), (s, rank)
        a, b = got[0][0][s + 1], got[1][0][s + 1]
        assert np.array_equal(a["cand"], b["cand"]) and np.array_equal(a["gbuf"], b["gbuf"]), s
        assert np.array_equal(a["params"], b["params"]), s                           # the replicas stay bit-identical
        assert not np.array_equal(a["params"], got[0][0][s]["params"])
    print(f"two ranks captured {negatives}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    assert mode == ic.ALL or worst["blind"] > 1e-3                                     # the classes matter on these rows
    assert got[0][2] == got[1][2] == len(ROWS)


@pytest.mark.parametrize("negatives", NAMES)
def test_call_record_of_a_rank_is_four_groups_and_three_collectives(negatives):
    """capture_inbatch_epoch_steps' docstring with several ranks: one warm-up of the forward body outside capture, then per replay
    [MFCC front-end, encoder forward] all-gather of the candidates (and of the classes beside it) [head] all-reduce of the candidate
    gradients [encoder backward] all-reduce of [gradients | loss] [Adam + row fetch] -- and nothing else, on either rank."""
    mode = ic.MODES[negatives]
    n_arena = var_amd.N_PARAMS + 1
    head = ("inbatch_ex", B, 4 * B, 1.0 / (2 * B), mode) if mode else ("inbatch", B, 4 * B, 1.0 / (2 * B))
    fwd = [("mfcc", 2 * B), ("encoder_fwd", B)]
    want = list(fwd)
    for k in range(1, len(ROWS) + 1):
        want += fwd
        want += [("allgather", (2 * B, 3))] + ([("allgather", (2 * B,))] if mode else [])
        want += [head, ("allreduce_sum", (4 * B, 3)), ("encoder_bwd",), ("allreduce_sum", (n_arena,)), ("adam_graph", k)]
    for rank, (_steps, calls, _count) in enumerate(_two_ranks(negatives)):
        assert calls == want, (rank, calls)

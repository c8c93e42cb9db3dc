"""The clip cache of the MFCC front-end (include/var_hip.h: var_mfcc_cache_bind / _unbind; VARTrainer(cache_clips=...)):
a pool clip's features are computed once and served to repeated draws.  Frames are computed independently of their tile
neighbours, so a served slot must hold the very bits a live computation gives: every comparison here is torch.equal
against the same call, or the same trainer, without the cache."""
import os
import types

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROWS, WIDTH = 6, 16000
CACHED_LENS = [16000, 12345, 8000, 160, 1, -1]


def _load(golden_dir, name):
    return dict(np.load(os.path.join(golden_dir, name)))


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


@pytest.fixture(scope="module")
def op(var_amd):
    """Pool of 6 rows x 16000 samples, its cache (row 5 not cached: length -1, features NaN) and a runner of var_mfcc with
    or without a binding."""
    from var_amd._lib import Context, ptr
    ctx = Context.get(0)
    g = torch.Generator(device="cuda").manual_seed(5)
    pcm = torch.randint(-20000, 20000, (ROWS, WIDTH), dtype=torch.int16, device="cuda", generator=g)
    clens = torch.tensor(CACHED_LENS, dtype=torch.int32, device="cuda")

    def run(lens, clip_index, frames=100, bind=None, src=pcm):
        """bind = (pcm, out_frames, cache_lens, cache_feats) or None"""
        lens = torch.tensor(lens, dtype=torch.int32, device="cuda")
        idx = None if clip_index is None else torch.tensor(clip_index, dtype=torch.int32, device="cuda")
        n = lens.numel()
        out = torch.full((n, 1, frames, 40), 7.0, dtype=torch.float32, device="cuda")
        if bind is not None:
            bp, bf, bl, bfeat = bind
            ctx.check(ctx.lib.var_mfcc_cache_bind(ctx.handle, ptr(bp), int(bp.shape[0]), bp.stride(0), bf, ptr(bl), ptr(bfeat)),
                      "var_mfcc_cache_bind")
        try:
            ctx.check(ctx.lib.var_mfcc(ctx.handle, ctx.stream(), ptr(src), ptr(lens), ptr(idx), n, src.stride(0), frames,
                                       ptr(out)), "var_mfcc")
        finally:
            if bind is not None:
                ctx.check(ctx.lib.var_mfcc_cache_unbind(ctx.handle), "var_mfcc_cache_unbind")
        torch.cuda.synchronize()
        return out

    feats = run([max(n, 0) for n in CACHED_LENS], None).reshape(ROWS, 100, 40).clone()
    feats[5] = float("nan")                                  # never served: a copy of it would show
    return types.SimpleNamespace(run=run, pcm=pcm, clens=clens, feats=feats, bind=(pcm, 100, clens, feats))


# (lens, clip_index) per case; "mixed" puts a served slot next to a live one of the same row with another length, an empty
# one, a row whose cached length is -1 and a repeated row: with 100 frames per clip and 16 per tile, tiles straddle
# served | live (slots 0|1, 5|6), live | dead (inside slot 1: 76 live frames), served | dead (2|3), dead | served (3|4)
CASES = {
    "mixed": ([16000, 12000, 12345, 0, 8000, 16000, 160, 160, 1], [0, 0, 1, 1, 2, 5, 3, 3, 4]),
    "all_served": ([16000, 12345, 8000, 160, 1, 16000, 8000], [0, 1, 2, 3, 4, 0, 2]),
    "all_live": ([15999, 12344, 8001, 161, 2, 16000, 320], [0, 1, 2, 3, 4, 5, 0]),
    "no_index": ([16000, 12345, 100, 0, 1, 16000], None),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_bound_call_equals_unbound_call(op, case):
    lens, idx = CASES[case]
    want = op.run(lens, idx)
    got = op.run(lens, idx, bind=op.bind)
    assert torch.isfinite(want).all() and not (want == 7.0).any()       # every element written
    assert torch.equal(got, want)


def test_served_slots_are_copies_of_the_cache(op):
    """The binding is really used: with the cache's rows replaced by a pattern, served slots show the pattern and live or
    empty slots do not."""
    lens, idx = CASES["mixed"]
    marked = torch.arange(ROWS * 100 * 40, dtype=torch.float32, device="cuda").reshape(ROWS, 100, 40) + 0.5
    got = op.run(lens, idx, bind=(op.pcm, 100, op.clens, marked)).reshape(len(lens), 100, 40)
    want = op.run(lens, idx).reshape(len(lens), 100, 40)
    for i, (n, r) in enumerate(zip(lens, idx)):
        served = n > 0 and n == CACHED_LENS[r]
        assert torch.equal(got[i], marked[r] if served else want[i]), i


def test_other_frame_count_or_other_pool_is_not_served(op):
    """A binding holds for its pool pointer, stride and frame count only: the cache is poisoned with NaN and must not show."""
    poison = torch.full_like(op.feats, float("nan"))
    bind = (op.pcm, 100, op.clens, poison)
    lens, idx = CASES["all_served"]
    want50 = op.run(lens, idx, frames=50)
    assert torch.equal(op.run(lens, idx, frames=50, bind=bind), want50) and torch.isfinite(want50).all()
    other = op.pcm.clone()
    want = op.run(lens, idx, src=other)
    assert torch.equal(op.run(lens, idx, src=other, bind=bind), want) and torch.isfinite(want).all()
    assert not torch.isfinite(op.run(lens, idx, bind=bind)).all()       # (the same call on the bound pool is served)


def test_bind_refuses_bad_arguments(op):
    from var_amd._lib import Context, ptr
    ctx = Context.get(0)
    lib, h = ctx.lib, ctx.handle
    assert lib.var_mfcc_cache_bind(h, None, ROWS, WIDTH, 100, ptr(op.clens), ptr(op.feats)) != 0
    assert lib.var_mfcc_cache_bind(h, ptr(op.pcm), 0, WIDTH, 100, ptr(op.clens), ptr(op.feats)) != 0
    assert lib.var_mfcc_cache_bind(h, ptr(op.pcm), ROWS, WIDTH, 100, None, ptr(op.feats)) != 0
    assert lib.var_mfcc_cache_bind(h, ptr(op.pcm), 1 << 26, WIDTH, 100, ptr(op.clens), ptr(op.feats)) != 0
    assert lib.var_mfcc_cache_unbind(h) == 0


# ---- the trainer: captured steps with and without the cache ----
def _cfg():
    return types.SimpleNamespace(img_dim=(3, 84, 84), sound_dim=(1, 100, 40), representationDim=3)


def _snap(tr, model):
    torch.cuda.synchronize()
    return tr.loss.clone(), tr.grads.clone(), model.flat_parameters().detach().clone()


@pytest.fixture(scope="module")
def scenario(var_amd):
    """Pools and tables shared by the cached and the uncached run (B = 16, 4 clips per class, ragged lengths).  "full":
    64 triplets, 3 rows; "tail": 40 triplets = 16 / 16 / 8.  table2: one length changed by hand (that slot goes live inside
    the graph) in row 0, and row 1's first slot draws clip 2 at its cached length (the staleness step)."""
    B = 16
    out = {}
    for name, n_items in (("full", 64), ("tail", 40)):
        pool = var_amd.SyntheticTripletPool(n_items, hw=84, seed=11, clips_per_class=4, ragged_lens=True).freeze_pairs()
        if name == "full":
            table, spe, bt = pool.index_table(B, 3)[:3].contiguous(), None, 0
        else:
            table, spe, bt = pool.epoch_index_table(B, drop_last=False), 3, 8
            assert table.shape[0] == 3
        t2 = table.flip(0).contiguous() if name == "full" else table.clone()
        lens0 = t2[0, 3 * B:5 * B]
        k = int(torch.nonzero(lens0 > 320)[0])
        t2[0, 3 * B + k] -= 160
        t2[1, B] = 2
        t2[1, 3 * B] = int(pool.clip_len[2])
        out[name] = types.SimpleNamespace(pool=pool, clips0=pool.clips.clone(), table=table, table2=t2, spe=spe, bt=bt, B=B)
    return out


def _run(var_amd, golden_dir, sc, **trainer_kw):
    sd = _load(golden_dir, "kuka_weights.npz")
    pool, B = sc.pool, sc.B
    pool.clips.copy_(sc.clips0)
    model = var_amd.VARPretextNet(_cfg())
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to("cuda")
    tr = var_amd.VARTrainer(model, lr=1e-3, weight_decay=1e-6, **trainer_kw)
    kw = dict(steps_per_epoch=sc.spe, tail_batch=sc.bt) if sc.bt else {}
    replay, load_table = tr.capture_epoch_steps(pool.images, pool.clips, B, sc.table, clip_len=pool.clip_len, **kw)
    snaps = []
    for _ in range(4):                                       # the 4th replay wraps to row 0
        replay()
        snaps.append(_snap(tr, model))
    load_table(sc.table2)
    replay()                                                 # row 0: one slot's length differs from its clip's cached one
    snaps.append(_snap(tr, model))
    pool.clips[2].add_(1)                                    # the pool changes under the cache
    replay()                                                 # row 1 draws clip 2
    snaps.append(_snap(tr, model))
    pool.clips.copy_(sc.clips0)
    return tr, snaps


@pytest.mark.parametrize("name", ["full", "tail"])
def test_replayed_steps_equal_the_uncached_trainer(var_amd, golden_dir, scenario, name):
    """Four replays incl. the table wrap, a table with one length changed by hand, and pool.clips[2].add_(1) between two
    replays: loss, gradients and parameters after every step equal those of a trainer with cache_clips=False."""
    sc = scenario[name]
    tr_c, got = _run(var_amd, golden_dir, sc)
    assert len(tr_c._clip_caches) == 1
    cache = next(iter(tr_c._clip_caches.values()))
    assert torch.equal(cache["lens"], sc.pool.clip_len)
    tr_u, want = _run(var_amd, golden_dir, sc, cache_clips=False)
    assert len(tr_u._clip_caches) == 0
    for s, (g, w) in enumerate(zip(got, want)):
        for what, a, b in zip(("loss", "grads", "params"), g, w):
            assert torch.equal(a, b), (s, what, float((a - b).abs().max()))
    assert not torch.equal(got[-1][2], got[-2][2])


def test_refill_after_a_write_to_the_pool(var_amd, golden_dir, scenario):
    """The version check itself: a write to the pool refills the same buffers with the new clip's features."""
    sc = scenario["full"]
    pool = sc.pool
    pool.clips.copy_(sc.clips0)
    model = var_amd.VARPretextNet(_cfg()).to("cuda")
    tr = var_amd.VARTrainer(model)
    cache = tr._clip_cache(pool.clips, pool.clip_len)
    feats, before = cache["feats"], cache["feats"].clone()
    assert tr._clip_cache(pool.clips, pool.clip_len) is cache
    pool.clips[2].add_(1)
    tr._refresh_clips(cache)
    torch.cuda.synchronize()
    assert cache["feats"] is feats and cache["feats"].data_ptr() == feats.data_ptr()
    assert not torch.equal(feats[2], before[2]) and torch.equal(feats[3], before[3])
    want = var_amd.mfcc(pool.clips, pool.clip_len).reshape(-1, 100, 40)
    assert torch.equal(feats, want)
    pool.clips.copy_(sc.clips0)


def test_pool_above_the_byte_cap_runs_uncached(var_amd, golden_dir, scenario):
    sc = scenario["full"]
    pool, B = sc.pool, sc.B
    pool.clips.copy_(sc.clips0)
    sd = _load(golden_dir, "kuka_weights.npz")
    res = []
    for kw in (dict(clip_cache_bytes=pool.clips.shape[0] * 16004 - 1), dict(cache_clips=False)):
        model = var_amd.VARPretextNet(_cfg())
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        model = model.to("cuda")
        tr = var_amd.VARTrainer(model, lr=1e-3, **kw)
        assert tr._clip_cache(pool.clips, pool.clip_len) is None
        r = sc.table[0]
        tr.step_from_dataset(pool.images, r[:B], pool.clips, r[B:3 * B], r[3 * B:], clip_len=pool.clip_len)
        assert len(tr._clip_caches) == 0
        res.append(_snap(tr, model))
    assert all(torch.equal(a, b) for a, b in zip(*res))
    model = var_amd.VARPretextNet(_cfg()).to("cuda")
    assert var_amd.VARTrainer(model, clip_cache_bytes=pool.clips.shape[0] * 16004)._clip_cache(pool.clips) is not None

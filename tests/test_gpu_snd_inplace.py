"""Served clips read in place by the sound CNN (csrc/clip_src.h): when the training step runs the front-end itself under a
clip cache, snd_fwd_kernel and snd_wgrad_kernel take a served slot's features from its cache row and an empty slot's from
nowhere, and the front-end neither copies nor zeroes those slots.  Bit 7 of var_set_streams keeps the copy: the same
kernels reading the same bits out of the feature buffer, so every comparison here is torch.equal between a call, or a
trainer, under mask 3 and the same under mask 3 | 128."""
import os
import types

import numpy as np
import pytest
import torch

from tests.test_gpu_mfcc_cache import CACHED_LENS, ROWS, WIDTH, op, var_amd  # noqa: F401  (pool, cache and module fixtures)

pytestmark = pytest.mark.gpu

IN_PLACE, COPY = 3, 3 | 128
SND_T = (48, 23, 11, 5)                                     # frames of sact1..4, 32 channels each

# (length, pool row) per slot; B = 5 puts slots 0-3 | 4-7 | 8-9 into the three forward workgroups: the first holds a served, a
# live and an empty clip together, the last is partial.  Row 0 at its cached length is drawn twice; row 0 again at another
# length is live; row 1 (12345) and row 2 (8000) are served short -- their zero tail rows come from the cache; row 5 is
# cached with -1 and stays live at any length; row 3 is drawn empty and at twice its cached length.
MIXED = [(16000, 0), (12000, 0), (0, 1), (12345, 1), (16000, 5), (16000, 0), (8000, 2), (0, 3), (320, 3), (1, 4)]
# clip_index = NULL: the slot is the row; rows 6.. lie outside the 6-row cache and are live (or empty)
NO_INDEX = [16000, 12345, 0, 160, 2, 16000, 16000, 0, 8000, 15999]
SERVED_OR_EMPTY = [(16000, 0), (0, 2), (12345, 1), (8000, 2), (160, 3), (0, 0), (1, 4), (16000, 0), (0, 5), (8000, 2)]


def _slots(pattern, B):
    """2 B slots cycling through the pattern (B = 5: the pattern itself)."""
    return [pattern[i % len(pattern)] for i in range(2 * B)]


@pytest.fixture(scope="module")
def rig(var_amd, op, golden_dir):
    """The cache test's 6-row pool and cache, inside a pool of 70 rows (clip_index = NULL needs a row per slot), a model with
    the golden weights and a runner of one var_arm_loss_grad_pcm call under a stream mask."""
    from var_amd._lib import Context, ptr
    assert {16000, 12345, 8000, -1} <= set(CACHED_LENS)
    ctx = Context.get(0)
    g = torch.Generator(device="cuda").manual_seed(9)
    pcm = torch.cat([op.pcm, torch.randint(-20000, 20000, (64, WIDTH), dtype=torch.int16, device="cuda", generator=g)])
    images = torch.randint(0, 256, (40, 3, 84, 84), dtype=torch.uint8, device="cuda", generator=g)
    sd = dict(np.load(os.path.join(golden_dir, "kuka_weights.npz")))
    model = var_amd.VARPretextNet(types.SimpleNamespace(img_dim=(3, 84, 84), sound_dim=(1, 100, 40), representationDim=3))
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to("cuda")
    tr = var_amd.VARTrainer(model, cache_clips=False)       # (the binding is made by hand below)
    flat = model.flat_parameters()

    def step(B, lens, rows, mask, bind=True, later_bwd=None):
        """One fused step at batch B; returns loss, gradients, sact1..4 of the 2 B clips and, with later_bwd = (ga, gp, gn),
        the gradients of an explicit var_arm_encoder_bwd of the same forward."""
        lens_t = torch.tensor(lens, dtype=torch.int32, device="cuda")
        idx_t = None if rows is None else torch.tensor(rows, dtype=torch.int32, device="cuda")
        img_idx = torch.arange(B, dtype=torch.int32, device="cuda")
        ctx.ensure_plan(B, 84)
        tr._bind()
        tr.gbuf.fill_(7.0)
        old = ctx.set_streams(mask)
        if bind:
            ctx.check(ctx.lib.var_mfcc_cache_bind(ctx.handle, ptr(pcm), ROWS, pcm.stride(0), 100, ptr(op.clens), ptr(op.feats)),
                      "var_mfcc_cache_bind")
        try:
            ctx.check(ctx.lib.var_arm_loss_grad_pcm(ctx.handle, ctx.stream(), ptr(flat), ptr(images), 1, images.stride(0),
                                                    ptr(img_idx), ptr(pcm), pcm.stride(0), ptr(idx_t), ptr(lens_t), B, 84, 1.0,
                                                    1.0 / B, ptr(tr.gbuf), tr._loss_ptr(), None), "var_arm_loss_grad_pcm")
        finally:
            if bind:
                ctx.check(ctx.lib.var_mfcc_cache_unbind(ctx.handle), "var_mfcc_cache_unbind")
            ctx.set_streams(old)
        torch.cuda.synchronize()
        out = {"loss": tr.loss.clone(), "grads": tr.grads.clone()}
        for l, t in enumerate(SND_T, 1):
            out[f"sact{l}"] = ctx.debug_buffer(f"sact{l}", count=2 * B * 32 * t)
        if later_bwd is not None:
            g2 = torch.full_like(tr.gbuf, 7.0)
            ctx.check(ctx.lib.var_arm_encoder_bwd(ctx.handle, ctx.stream(), ptr(flat), ptr(later_bwd[0]), ptr(later_bwd[1]),
                                                  ptr(later_bwd[2]), ptr(g2)), "var_arm_encoder_bwd")
            torch.cuda.synchronize()
            out["later_grads"] = g2[:var_amd.N_PARAMS].clone()
        return out

    return types.SimpleNamespace(ctx=ctx, step=step, pcm=pcm)


def _assert_same(got, want):
    assert got.keys() == want.keys()
    for k in want:
        assert torch.isfinite(want[k]).all(), k
        assert torch.equal(got[k], want[k]), (k, float((got[k] - want[k]).abs().max()))
    assert float(want["grads"].abs().max()) > 0 and not (want["grads"] == 7.0).any()


def _lens_rows(slots):
    return [n for n, _ in slots], [r for _, r in slots]


def test_mixed_batch(rig):
    """B = 5: served full, served short, live, empty, a row cached with -1 and a repeated row, in three forward workgroups and
    ten weight-gradient slabs."""
    lens, rows = _lens_rows(_slots(MIXED, 5))
    _assert_same(rig.step(5, lens, rows, IN_PLACE), rig.step(5, lens, rows, COPY))


def test_no_gather_index(rig):
    """clip_index = NULL: the slot is the row."""
    _assert_same(rig.step(5, NO_INDEX, None, IN_PLACE), rig.step(5, NO_INDEX, None, COPY))


@pytest.mark.parametrize("B", [32, 33])
def test_stream_plans(rig, B):
    """B = 33: the sound branch on the side stream (fork_ok); B = 32: everything on the caller's stream."""
    lens, rows = _lens_rows(_slots(MIXED, B))
    _assert_same(rig.step(B, lens, rows, IN_PLACE), rig.step(B, lens, rows, COPY))


def test_served_and_empty_slots_are_not_copied(rig):
    """After a copying step has filled the feature buffer, an in-place step over another batch whose slots are all served or
    empty leaves the buffer as it was -- and computes what the copying form computes for that batch."""
    lens_b, rows_b = _lens_rows(SERVED_OR_EMPTY)
    want = rig.step(5, lens_b, rows_b, COPY)
    lens_a, rows_a = _lens_rows(_slots(MIXED, 5))
    rig.step(5, lens_a, rows_a, COPY)
    before = rig.ctx.debug_buffer("mfcc", count=10 * 100 * 40)
    got = rig.step(5, lens_b, rows_b, IN_PLACE)
    after = rig.ctx.debug_buffer("mfcc", count=10 * 100 * 40)
    assert torch.equal(after, before)
    assert not torch.equal(before[:4000], torch.zeros_like(before[:4000]))        # (slot 0 of the first batch was served: copied)
    _assert_same(got, want)
    # the copying form does rewrite it: the check above can fail
    rig.step(5, lens_b, rows_b, COPY)
    assert not torch.equal(rig.ctx.debug_buffer("mfcc", count=10 * 100 * 40), before)


def test_later_backward_reads_the_same_rows(rig):
    """An explicit var_arm_encoder_bwd after the fused step (the cache long unbound) reads the forward's sources again."""
    g = torch.Generator(device="cuda").manual_seed(3)
    gs = [torch.randn((5, 3), dtype=torch.float32, device="cuda", generator=g) for _ in range(3)]
    lens, rows = _lens_rows(_slots(MIXED, 5))
    got = rig.step(5, lens, rows, IN_PLACE, later_bwd=gs)
    want = rig.step(5, lens, rows, COPY, later_bwd=gs)
    _assert_same(got, want)
    assert not torch.equal(want["later_grads"], want["grads"])


def test_without_a_binding(rig):
    """No cache bound: the same kernels with a ClipSrc that names no cache -- every slot is read from the feature buffer."""
    lens, rows = _lens_rows(_slots(MIXED, 5))
    got, want = rig.step(5, lens, rows, IN_PLACE, bind=False), rig.step(5, lens, rows, COPY, bind=False)
    _assert_same(got, want)
    _assert_same(rig.step(5, lens, rows, IN_PLACE), want)            # (and the cache changes no bit)


def _trainer_run(var_amd, golden_dir, pool, B, tables, mask, **trainer_kw):
    from var_amd._lib import Context
    ctx = Context.get(0)
    sd = dict(np.load(os.path.join(golden_dir, "kuka_weights.npz")))
    old = ctx.set_streams(mask)
    try:
        model = var_amd.VARPretextNet(types.SimpleNamespace(img_dim=(3, 84, 84), sound_dim=(1, 100, 40), representationDim=3))
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        model = model.to("cuda")
        tr = var_amd.VARTrainer(model, lr=1e-3, weight_decay=1e-6, **trainer_kw)
        replay, load_table = tr.capture_epoch_steps(pool.images, pool.clips, B, tables[0], clip_len=pool.clip_len)
        snaps = []
        for _ in range(3):
            replay()
            torch.cuda.synchronize()
            snaps.append((tr.loss.clone(), model.flat_parameters().detach().clone()))
        load_table(tables[1])
        replay()
        torch.cuda.synchronize()
        snaps.append((tr.loss.clone(), model.flat_parameters().detach().clone()))
        return snaps, len(tr._clip_caches)
    finally:
        ctx.set_streams(old)


def test_replayed_steps(var_amd, golden_dir):
    """capture_epoch_steps at B = 48, H = 84 (the device-side hand-over is active): rows that differ in which slots are served,
    live (their length changed by hand) or empty; three replays, a new table, one more replay."""
    from var_amd._lib import Context
    ctx = Context.get(0)
    B = 48
    pool = var_amd.SyntheticTripletPool(4 * B, hw=84, seed=5, clips_per_class=4, ragged_lens=True).freeze_pairs()
    table = pool.index_table(B, 4)[:4].contiguous()
    for r in range(4):                                        # every row: a different handful of slots goes live
        lens = table[r, 3 * B:5 * B]
        live = torch.nonzero(lens > 320).reshape(-1)[r::7][:6]
        table[r, 3 * B + live] -= 160
        kinds = (lens == 0).sum().item(), len(live)
        assert kinds[0] > 0 and kinds[1] > 0 and kinds[0] + kinds[1] < 2 * B, kinds
    table2 = table.flip(0).contiguous()
    before = ctx.join_timeouts()
    got, n_caches = _trainer_run(var_amd, golden_dir, pool, B, (table, table2), IN_PLACE)
    assert n_caches == 1
    want, _ = _trainer_run(var_amd, golden_dir, pool, B, (table, table2), COPY)
    assert ctx.join_timeouts() == before
    for s, ((gl, gp), (wl, wp)) in enumerate(zip(got, want)):
        assert torch.isfinite(wl).all() and torch.equal(gl, wl), (s, float(gl), float(wl))
        assert torch.equal(gp, wp), (s, float((gp - wp).abs().max()))
    assert not torch.equal(want[-1][1], want[-2][1])

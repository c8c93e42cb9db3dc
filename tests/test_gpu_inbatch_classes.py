"""GPU checks of the class-aware in-batch head (csrc/inbatch.hip: var_inbatch_loss_fwd_bwd_ex) and of the trainers that carry the
classes to it.  The kernels alone, through the C ABI with every array between 64 sentinel elements on each side (the Buf of
tests/test_gpu_step_tail.py): mode 0 and the modes whose masks select nothing against the label-blind entry bit for bit; modes 1
and 2 against the float64 restatement of tests/inbatch_classes_cpu.py within four times torch fp32's own distance from float64 at
the same case (classes_distance: the largest over 20 seeded draws, per output); rows left alone with their positive; what a
masked candidate receives; the refusals.  Then VARTrainer.step_inbatch / capture_inbatch_epoch_steps and IthorTrainer.step_inbatch
with classes, and two ranks on one device.  No bound here was taken from what the kernels give.
Seen on an MI355X, the largest distance over all parity cases beside the range of its bounds: loss 1.0e-7 (3.3e-7 .. 6.2e-7),
g_anchor 2.5e-7 at tau 0.1 (9.4e-7 .. 1.4e-6), 1.6e-6 at tau 0.01 (6.0e-6) and 6.6e-7 at tau 1 (1.1e-6, 2.7e-6), g_cand 2.6e-7
at tau 0.1 and 1 (5.9e-7 .. 1.4e-6) and 1.2e-6 at tau 0.01 (7.7e-6, 7.9e-6): the kernels sit at 0.4 of the bounds or below; the rows left
alone with their positive give a loss of exactly 0."""
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from tests import inbatch_classes_cpu as ic
from tests import step_tail_cpu as st
from tests.test_gpu_step_tail import ERR_ARG, Buf, bits, last_error, run_inbatch

pytestmark = pytest.mark.gpu

MODES = (ic.OTHER_CLASS, ic.MULTI_POSITIVE)
NAMES = {ic.ALL: "all", ic.OTHER_CLASS: "other_class", ic.MULTI_POSITIVE: "multi_positive"}
OUT = ("loss", "ga", "gc")


@pytest.fixture(scope="module")
def ctx():
    import var_amd  # noqa: F401
    from var_amd._lib import Context
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return Context.get(0)


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def run_ex(ctx, a, cand, t, y, z, tau, inv, mode, null_classes=False):
    B, M = a.shape[0], cand.shape[0]
    b = {"a": Buf(a), "c": Buf(cand), "t": Buf(t, dtype=torch.int32), "y": Buf(y, dtype=torch.int32), "z": Buf(z, dtype=torch.int32),
         "scratch": Buf(n=3 * B), "loss": Buf(n=1), "ga": Buf(n=3 * B), "gc": Buf(n=3 * M)}
    rc = ctx.lib.var_inbatch_loss_fwd_bwd_ex(ctx.handle, None, b["a"].ptr, b["c"].ptr, b["t"].ptr, None if null_classes else b["y"].ptr,
                                             None if null_classes else b["z"].ptr, B, M, tau, inv, mode, b["scratch"].ptr,
                                             b["loss"].ptr, b["ga"].ptr, b["gc"].ptr)
    assert rc == 0, last_error(ctx)
    assert all(b[k].untouched() for k in "actyz") and all(b[k].pads_ok() for k in ("scratch", "loss", "ga", "gc"))
    return {"loss": b["loss"].host(), "ga": b["ga"].host().reshape(B, 3), "gc": b["gc"].host().reshape(M, 3)}


def same_bits(x, y):
    return all(np.array_equal(bits(x[k]), bits(y[k])) for k in OUT)


def distances(got, ref):
    return {k: float(np.abs(got[k].astype(np.float64) - ref[k]).max()) / st.scale(ref[k]) for k in OUT}


# ---- against the label-blind entry, bit for bit ------------------------------------------------------------------------------
@pytest.mark.parametrize("null_classes", [True, False])
@pytest.mark.parametrize("B, M", [(1, 1), (5, 65), (257, 130)])
def test_mode_all_is_the_old_entry_bit_for_bit(ctx, B, M, null_classes):
    a, cand, t, y, z = ic.class_inputs(B, M, 800 + B + M)
    old = run_inbatch(ctx, a, cand, t, 0.1, 1.0 / B)
    assert same_bits(run_ex(ctx, a, cand, t, y, z, 0.1, 1.0 / B, ic.ALL, null_classes), old)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B, M", [(5, 65), (257, 130)])
def test_modes_without_a_shared_class_are_the_old_entry_bit_for_bit(ctx, B, M, mode):
    """Unique candidate classes, y_i = z_{t(i)}: N_i is every column and P_i = { t(i) } -- also for anchors 2 and 3, which share a
    column."""
    a, cand, t = st.inbatch_inputs(B, M, 810 + B + M)
    assert t[2] == t[3]
    z = np.random.default_rng(B + M).permutation(M).astype(np.int32) + 7
    old = run_inbatch(ctx, a, cand, t, 0.1, 1.0 / B)
    assert same_bits(run_ex(ctx, a, cand, t, z[t].copy(), z, 0.1, 1.0 / B, mode), old)


# ---- against float64 ---------------------------------------------------------------------------------------------------------
def check_parity(ctx, B, M, tau, inv, mode, seed):
    a, cand, t, y, z = ic.class_inputs(B, M, seed)
    assert ic.min_negatives(t, y, z) >= ic.MIN_NEGATIVES
    assert ic.negatives_mask(t, y, z).sum() < B * M and ic.positives_mask(t, y, z).sum() > B       # the masks select something
    got = run_ex(ctx, a, cand, t, y, z, tau, inv, mode)
    assert all(np.isfinite(got[k]).all() for k in OUT)
    ref = ic.classes64(a, cand, t, y, z, st.f32(tau), st.f32(inv), mode)
    D = ic.classes_distance(B, M, tau, inv, mode)
    d = distances(got, ref)
    print(f"in-batch {NAMES[mode]} ({B},{M}) tau={tau} inv_count={inv:.3e}: " + " ".join(f"{k} {d[k]:.2e}/{4 * D[k]:.2e}" for k in OUT))
    assert all(d[k] <= 4 * D[k] for k in OUT), d
    assert same_bits(run_ex(ctx, a, cand, t, y, z, tau, inv, mode), got)                            # a repeat run: the same bits
    return a, cand, t, y, z, ref


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("B, M", [(3, 63), (4, 64), (5, 65), (257, 130), (300, 70)])
def test_against_float64_at_the_wave_and_block_edges(ctx, B, M, mode):
    check_parity(ctx, B, M, 0.1, 1.0 / B, mode, 500 + B + M)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("tau", [0.01, 1.0])
def test_temperatures(ctx, tau, mode):
    check_parity(ctx, 5, 65, tau, 1.0 / 5, mode, 670)


@pytest.mark.parametrize("mode", MODES)
def test_global_inv_count_and_row_split(ctx, mode):
    B, M = 257, 130
    check_parity(ctx, 5, 65, 0.1, 1.0 / 20, mode, 700)
    a, cand, t, y, z, ref = check_parity(ctx, B, M, 0.1, 1.0 / B, mode, 701)
    parts = [run_ex(ctx, a[s], cand, t[s], y[s], z, 0.1, 1.0 / B, mode) for s in (slice(0, 128), slice(128, B))]
    whole = {"loss": parts[0]["loss"].astype(np.float64) + parts[1]["loss"], "ga": np.concatenate([parts[0]["ga"], parts[1]["ga"]]),
             "gc": parts[0]["gc"].astype(np.float64) + parts[1]["gc"]}
    D = ic.classes_distance(B, M, 0.1, 1.0 / B, mode)
    d = distances(whole, ref)
    print(f"in-batch {NAMES[mode]} (257,130) as rows 0..127 + 128..256: " + " ".join(f"{k} {d[k]:.2e}/{4 * D[k]:.2e}" for k in OUT))
    assert all(d[k] <= 4 * D[k] for k in OUT), d


# ---- rows left alone with their positive --------------------------------------------------------------------------------------
def check_lone_positive(ctx, a, cand, t, y, z, mode, label):
    """softmax = 1 on the positive: no gradient; the loss is d/tau - d/tau, zero within the rounding of d/tau (the M == 1 rule of
    tests/test_gpu_step_tail.py)."""
    B, tau, inv = a.shape[0], 0.1, 1.0 / a.shape[0]
    got = run_ex(ctx, a, cand, t, y, z, tau, inv, mode)
    d64 = np.linalg.norm(a.astype(np.float64) - cand[t].astype(np.float64) + st.PD_EPS, axis=1) / st.f32(tau)
    bound = 4 * 0.5 * float(st.ulp32(d64.max())) * B * st.f32(inv)
    print(f"in-batch {NAMES[mode]} {label}: |loss| {abs(float(got['loss'][0])):.2e}/{bound:.2e}")
    assert abs(float(got["loss"][0])) <= bound
    assert (got["ga"] == 0).all() and (got["gc"] == 0).all()


@pytest.mark.parametrize("B, M", [(4, 64), (64, 1)])
def test_other_class_with_one_class_leaves_every_row_alone_with_its_positive(ctx, B, M):
    a, cand, t = st.inbatch_inputs(B, M, 820 + B + M)
    check_lone_positive(ctx, a, cand, t, np.full(B, 3, np.int32), np.full(M, 3, np.int32), ic.OTHER_CLASS, f"({B},{M}) one class")


def test_smallest_shapes(ctx):
    a, cand, t = st.inbatch_inputs(1, 1, 830)
    check_lone_positive(ctx, a, cand, t, np.array([2], np.int32), np.array([4], np.int32), ic.MULTI_POSITIVE, "(1,1)")
    a, cand, t = st.inbatch_inputs(1, 2, 831)
    check_lone_positive(ctx, a, cand, t, np.array([1], np.int32), np.array([1, 1], np.int32), ic.OTHER_CLASS, "(1,2) both of the anchor's class")


def test_a_masked_candidate_receives_no_gradient(ctx):
    """Every anchor of class 2; candidate j of class 2, nobody's positive: its gradient is exactly zero, and with another class it
    is not."""
    B, M = 5, 65
    a, cand, t, _, z = ic.class_inputs(B, M, 840)
    y = np.full(B, 2, np.int32)
    j = int(np.setdiff1d(np.arange(M), t)[0])
    z[j] = 2
    masked = run_ex(ctx, a, cand, t, y, z, 0.1, 1.0 / B, ic.OTHER_CLASS)
    assert (masked["gc"][j] == 0).all()
    z[j] = 3
    scored = run_ex(ctx, a, cand, t, y, z, 0.1, 1.0 / B, ic.OTHER_CLASS)
    assert (scored["gc"][j] != 0).any()
    ref = ic.classes64(a, cand, t, y, z, st.f32(0.1), st.f32(1.0 / B), ic.OTHER_CLASS)
    assert np.abs(scored["gc"][j] - ref["gc"][j]).max() < 1e-5 * st.scale(ref["gc"])


# ---- refusals ----------------------------------------------------------------------------------------------------------------
def test_refusals_touch_nothing(ctx):
    a, cand, t, y, z = ic.class_inputs(5, 9, 1)
    b = {"a": Buf(a), "c": Buf(cand), "t": Buf(t, dtype=torch.int32), "y": Buf(y, dtype=torch.int32), "z": Buf(z, dtype=torch.int32),
         "scratch": Buf(n=15), "loss": Buf(n=1), "ga": Buf(n=15), "gc": Buf(n=27)}
    always = ("a", "c", "t", "scratch", "loss", "ga", "gc")
    cases = [dict(mode=m, **kw) for m in (0, 1, 2) for kw in [dict(tau=0.0), dict(tau=-0.1), dict(B=0), dict(M=0)] + [{k: None} for k in always]]
    cases += [dict(mode=-1), dict(mode=3)] + [dict(mode=m, **{k: None}) for m in (1, 2) for k in "yz"]
    for kw in cases:
        q = {k: (None if k in kw else b[k].ptr) for k in b}
        rc = ctx.lib.var_inbatch_loss_fwd_bwd_ex(ctx.handle, None, q["a"], q["c"], q["t"], q["y"], q["z"], kw.get("B", 5), kw.get("M", 9),
                                                 kw.get("tau", 0.1), 0.2, kw["mode"], q["scratch"], q["loss"], q["ga"], q["gc"])
        assert rc == ERR_ARG and last_error(ctx).startswith("var_inbatch_loss_fwd_bwd_ex:"), kw
    assert all(x.untouched() for x in b.values())


def test_python_front_checks_classes_and_modes(var_amd):
    a, cand, t, y, z = (cuda(x) for x in ic.class_inputs(5, 9, 2))
    bad = [dict(negatives="other_class"), dict(negatives="multi_positive"), dict(anchor_cls=y, negatives="other_class"),
           dict(anchor_cls=y, cand_cls=z, negatives="hard"), dict(anchor_cls=y.long(), cand_cls=z, negatives="other_class"),
           dict(anchor_cls=y, cand_cls=z.cpu(), negatives="other_class"), dict(anchor_cls=y, cand_cls=z[:8].contiguous(), negatives="all")]
    for kw in bad:
        with pytest.raises(var_amd.VarHipError):
            var_amd.inbatch_contrastive_loss(a, cand, t, 0.1, **kw)
    want = var_amd.inbatch_contrastive_loss(a, cand, t, 0.1)
    got = var_amd.inbatch_contrastive_loss(a, cand, t, 0.1, anchor_cls=y, cand_cls=z, negatives="all")
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    ref = ic.classes64(*(x.cpu().numpy() for x in (a, cand, t, y, z)), st.f32(0.1), st.f32(0.2), ic.MULTI_POSITIVE)
    loss, ga, gc = var_amd.inbatch_contrastive_loss(a, cand, t, 0.1, anchor_cls=y, cand_cls=z, negatives="multi_positive")
    assert abs(float(loss) - ref["loss"][0]) < 1e-5 * abs(ref["loss"][0])
    np.testing.assert_allclose(ga.cpu().numpy(), ref["ga"], atol=1e-5 * st.scale(ref["ga"]))
    np.testing.assert_allclose(gc.cpu().numpy(), ref["gc"], atol=1e-5 * st.scale(ref["gc"]))


# ---- the Kuka trainer -----------------------------------------------------------------------------------------------------------
def _cfg(h=84):
    return types.SimpleNamespace(img_dim=(3, h, h), sound_dim=(1, 100, 40), representationDim=3)


def kuka_model(var_amd, golden_dir):
    m = var_amd.VARPretextNet(_cfg())
    sd = dict(np.load(os.path.join(golden_dir, "kuka_weights.npz")))
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    return m.to("cuda")


def kuka_batch(golden_dir):
    fx = dict(np.load(os.path.join(golden_dir, "kuka_h84.npz")))
    return cuda(fx["image"]), cuda(fx["sound_positive"]), cuda(fx["sound_negative"])


def kuka_embeddings(tr, img, pos, neg):
    """var_arm_encoder_fwd's embeddings [image | pos | neg] (3, B, 3) of the trainer's model."""
    from var_amd._lib import ptr
    c, B = tr.ctx, img.shape[0]
    emb = torch.empty((3, B, 3), device="cuda")
    tr._bind()
    c.ensure_plan(B, 84)
    c.check(c.lib.var_arm_encoder_fwd(c.handle, c.stream(), ptr(tr.model.flat_parameters()), ptr(img), int(img.dtype == torch.uint8),
                                      img.stride(0), ptr(pos), ptr(neg), B, 84, ptr(emb[0]), ptr(emb[1]), ptr(emb[2]), None, None, 1),
            "var_arm_encoder_fwd")
    return emb


@pytest.mark.parametrize("negatives", ["other_class", "multi_positive"])
def test_kuka_step_with_classes_that_mask_nothing_is_the_step_without(var_amd, golden_dir, negatives):
    img, pos, neg = kuka_batch(golden_dir)
    B = img.shape[0]
    ma, mb = kuka_model(var_amd, golden_dir), kuka_model(var_amd, golden_dir)
    ta, tb = var_amd.VARTrainer(ma, lr=1e-3), var_amd.VARTrainer(mb, lr=1e-3)
    la = ta.step_inbatch(img, pos, neg, tau=0.1).clone()
    gt, sn = torch.arange(B, dtype=torch.int32, device="cuda"), torch.arange(B, 2 * B, dtype=torch.int32, device="cuda")
    lb = tb.step_inbatch(img, pos, neg, tau=0.1, classes=(gt, sn), negatives=negatives).clone()
    assert torch.equal(la, lb) and torch.equal(ta.grads, tb.grads) and torch.equal(ma.flat_parameters(), mb.flat_parameters())


@pytest.mark.parametrize("negatives", ["other_class", "multi_positive"])
def test_kuka_step_loss_is_the_head_on_the_forward_embeddings(var_amd, golden_dir, negatives):
    """(the fixture carries no labels: gt and sn are both drawn, sn never equal to gt as dataset.py:70-78 has it)"""
    img, pos, neg = kuka_batch(golden_dir)
    B = img.shape[0]
    rng = np.random.default_rng(5)
    gt_np = rng.integers(0, 3, B).astype(np.int32)
    sn_np = ((gt_np + rng.integers(1, 3, B)) % 3).astype(np.int32)
    gt, sn = cuda(gt_np), cuda(sn_np)
    m = kuka_model(var_amd, golden_dir)
    tr = var_amd.VARTrainer(m, lr=1e-3)
    emb = kuka_embeddings(tr, img, pos, neg)
    target = torch.arange(B, dtype=torch.int32, device="cuda")
    want, _, _ = var_amd.inbatch_contrastive_loss(emb[0], emb[1:].reshape(2 * B, 3), target, 0.1, 1.0 / B, gt, torch.cat([gt, sn]), negatives)
    blind, _, _ = var_amd.inbatch_contrastive_loss(emb[0], emb[1:].reshape(2 * B, 3), target, 0.1, 1.0 / B)
    p0 = m.flat_parameters().clone()
    got = tr.step_inbatch(img, pos, neg, tau=0.1, classes=(gt, sn), negatives=negatives)
    assert torch.equal(got, want) and not torch.equal(want, blind)
    assert float((m.flat_parameters() - p0).abs().max()) > 0


@pytest.mark.parametrize("negatives", ["other_class", "multi_positive"])
def test_kuka_replayed_step_with_classes_equals_eager(var_amd, golden_dir, negatives):
    """12 triplets at B = 4, four replays (the fourth wraps) against eager steps on the same rows, at the bounds tests/test_gpu_round2.py
    has for the label-blind replayed step."""
    B = 4
    pool = var_amd.SyntheticTripletPool(12, hw=84, seed=41, clips_per_class=4).freeze_pairs()
    gt_tab, sn_tab = pool.class_tables()
    assert gt_tab.dtype == torch.int32 and gt_tab.is_cuda and gt_tab.is_contiguous() and torch.equal(sn_tab.long(), pool.sn)
    table = pool.index_table(B, 3, drop_last=True)[:3].contiguous()
    mb = kuka_model(var_amd, golden_dir)
    tb = var_amd.VARTrainer(mb, lr=1e-3)
    replay, _ = tb.capture_inbatch_epoch_steps(pool.images, pool.clips, B, table, tau=0.1, classes=(gt_tab, sn_tab), negatives=negatives)
    losses_b = [float(replay().item()) for _ in range(4)]
    ma = kuka_model(var_amd, golden_dir)
    ta = var_amd.VARTrainer(ma, lr=1e-3)
    losses_a = []
    for s in range(4):
        r = table[s % 3]
        rows = r[:B].long()
        f = var_amd.mfcc(pool.clips, r[3 * B:], out_frames=100, clip_index=r[B:3 * B])
        losses_a.append(float(ta.step_inbatch(pool.images[rows].contiguous(), f[:B].contiguous(), f[B:].contiguous(), tau=0.1,
                                              classes=(gt_tab[rows].contiguous(), sn_tab[rows].contiguous()), negatives=negatives).item()))
    print(f"replayed {negatives}: eager {losses_a} replayed {losses_b}")
    assert np.allclose(losses_a, losses_b, rtol=0, atol=1e-5), (losses_a, losses_b)
    assert float((ma.flat_parameters() - mb.flat_parameters()).abs().max()) < 1e-4


# ---- the iTHOR trainer --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("negatives", ["all", "other_class", "multi_positive"])
def test_ithor_step_inbatch_is_forward_head_backward(var_amd, negatives):
    """B = 4, fp32: the step's loss is the head on the forward's embeddings and its gradient arena the one of _IthorFn forward,
    inbatch_contrastive_loss, backward -- bit for bit."""
    B = 4
    torch.manual_seed(123)
    m = var_amd.IthorVARPretextNet(types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 600, 40), representationDim=3)).to("cuda")
    g = torch.Generator().manual_seed(9)
    img = torch.randint(0, 256, (B, 3, 96, 96), dtype=torch.uint8, generator=g).cuda()
    pos, neg = ((torch.randn(B, 1, 600, 40, generator=g) * 4).cuda() for _ in range(2))
    gt = torch.tensor([0, 1, 0, 4], dtype=torch.int32, device="cuda")
    sn = torch.tensor([1, 0, 4, 0], dtype=torch.int32, device="cuda")
    kw = {} if negatives == "all" else dict(anchor_cls=gt, cand_cls=torch.cat([gt, sn]), negatives=negatives)
    d = m(img, pos, neg)
    emb = [d[k] for k in ("image_feat", "sound_feat_positive", "sound_feat_negative")]
    target = torch.arange(B, dtype=torch.int32, device="cuda")
    want, ga, gc = var_amd.inbatch_contrastive_loss(emb[0].detach(), torch.cat([emb[1], emb[2]]).detach(), target, 0.1, 1.0 / B, **kw)
    torch.autograd.backward(emb, [ga, gc[:B].contiguous(), gc[B:].contiguous()])
    auto = torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone()
    p0 = m.flat_parameters().clone()
    tr = var_amd.IthorTrainer(m, lr=1e-4)
    got = tr.step_inbatch(img, pos, neg, tau=0.1, **({} if negatives == "all" else dict(classes=(gt, sn), negatives=negatives)))
    assert torch.isfinite(got).all() and torch.equal(got, want)
    assert torch.equal(tr.grads, auto)
    assert tr.step_count == 1 and float((m.flat_parameters() - p0).abs().max()) > 0
    with pytest.raises(var_amd.VarHipError):
        tr.step_inbatch(img, pos, neg, negatives="other_class")
    with pytest.raises(var_amd.VarHipError):
        tr.step_inbatch(img, pos, neg, classes=(gt.long(), sn), negatives="other_class")


# ---- two ranks on one device ----------------------------------------------------------------------------------------------------
ITEMS = [list(range(0, 6)), list(range(11, 5, -1))]


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out):
    import torch.distributed as dist
    import var_amd
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(7 + rank)                                  # different initial weights: the trainer broadcasts rank 0's
    model = var_amd.VARPretextNet(_cfg()).to("cuda")
    tr = var_amd.VARTrainer(model, lr=1e-3)
    pool = var_amd.SyntheticTripletPool(12, hw=84, seed=3, clips_per_class=4).freeze_pairs()
    gt_tab, sn_tab = pool.class_tables()
    losses = []
    for items in ITEMS:
        n = len(items) // world
        mine = torch.tensor(items[rank * n:(rank + 1) * n], device="cuda")
        f = var_amd.mfcc(pool.clips, pool.len_tab[:, mine].reshape(-1), 100, pool.clip_tab[:, mine].reshape(-1))
        losses.append(float(tr.step_inbatch(pool.images[mine].contiguous(), f[:n].contiguous(), f[n:].contiguous(), tau=0.1,
                                            classes=(gt_tab[mine].contiguous(), sn_tab[mine].contiguous()), negatives="other_class").item()))
    out.put((rank, losses, model.flat_parameters().cpu().numpy().copy()))
    dist.destroy_process_group()


def test_two_ranks_other_class_equals_one_process_on_the_global_batch(var_amd):
    """In the manner of tests/test_gpu_dp2.py: two processes on cuda:0 exchanging through gloo, 3 triplets each, against ONE process
    scoring all 6 anchors on [p0 ; n0 ; p1 ; n1] with the classes ordered alike."""
    from var_amd._lib import ptr
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    port = _free_port()
    procs = [mpc.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=300) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    torch.manual_seed(7)
    model = var_amd.VARPretextNet(_cfg()).to("cuda")
    tr = var_amd.VARTrainer(model, lr=1e-3)
    pool = var_amd.SyntheticTripletPool(12, hw=84, seed=3, clips_per_class=4).freeze_pairs()
    gt_tab, sn_tab = pool.class_tables()
    want, blind = [], []
    for items in ITEMS:
        n = len(items) // 2
        i = torch.tensor(items, device="cuda")
        f = var_amd.mfcc(pool.clips, pool.len_tab[:, i].reshape(-1), 100, pool.clip_tab[:, i].reshape(-1))
        pos, neg = f[:2 * n], f[2 * n:]
        c, img = tr.ctx, pool.images[i].contiguous()
        emb = torch.empty((3, 2 * n, 3), device="cuda")
        tr._bind()
        c.ensure_plan(2 * n, 84)
        c.check(c.lib.var_arm_encoder_fwd(c.handle, c.stream(), ptr(model.flat_parameters()), ptr(img), 1, img.stride(0), ptr(pos), ptr(neg),
                                          2 * n, 84, ptr(emb[0]), ptr(emb[1]), ptr(emb[2]), None, None, 1), "fwd")
        cand = torch.cat([emb[1, :n], emb[2, :n], emb[1, n:], emb[2, n:]]).contiguous()
        gt, sn = gt_tab[i], sn_tab[i]
        ccls = torch.cat([gt[:n], sn[:n], gt[n:], sn[n:]]).contiguous()
        target = torch.cat([torch.arange(n), torch.arange(n) + 2 * n]).to(torch.int32).cuda()
        loss, ga, gc = var_amd.inbatch_contrastive_loss(emb[0], cand, target, tau=0.1, anchor_cls=gt.contiguous(), cand_cls=ccls,
                                                        negatives="other_class")
        blind.append(float(var_amd.inbatch_contrastive_loss(emb[0], cand, target, tau=0.1)[0].item()))
        gp = torch.cat([gc[:n], gc[2 * n:3 * n]]).contiguous()
        gn = torch.cat([gc[n:2 * n], gc[3 * n:]]).contiguous()
        c.check(c.lib.var_arm_encoder_bwd(c.handle, c.stream(), ptr(model.flat_parameters()), ptr(ga), ptr(gp), ptr(gn), ptr(tr.gbuf)), "bwd")
        tr.gbuf[var_amd.N_PARAMS:].copy_(loss)
        tr.adam()
        want.append(float(loss.item()))
    assert max(abs(w - b) for w, b in zip(want, blind)) > 1e-3       # the classes matter on these rows
    flat = model.flat_parameters().cpu().numpy()
    for _rank, losses, p in got:
        np.testing.assert_allclose(losses, want, atol=1e-5)
        d = np.abs(p - flat)
        assert d.max() < 1e-4 and np.mean(d < 2e-6) > 0.99, (d.max(), np.mean(d < 2e-6))
    assert np.array_equal(got[0][2], got[1][2])

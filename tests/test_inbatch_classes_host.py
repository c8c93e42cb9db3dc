"""Host side of the class-aware in-batch head: the float64 restatement of tests/inbatch_classes_cpu.py against plain double
loops, faults planted in it against its own yardstick, and the trainers' host logic around var_inbatch_loss_fwd_bwd_ex -- class
validation, the order [gt ; sn] of the candidate classes, their all-gather beside the embeddings', the class gather of the
replayed step by the index row -- driven on the CPU through tests/_oracle_ctx.py with the new entry bound to the restatement.
The kernels themselves are checked on the GPU (tests/test_gpu_inbatch_classes.py)."""
import os
import socket
import types

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import var_amd
from oracle import mfcc_np
from oracle.torch_oracle import KukaNetCPU
from tests import inbatch_classes_cpu as ic
from tests import step_tail_cpu as st
from tests._oracle_ctx import OracleContext, _arr, _Lib

NAMES = ("all", "other_class", "multi_positive")


# ---- the restatement itself --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [ic.ALL, ic.OTHER_CLASS, ic.MULTI_POSITIVE])
def test_restatement_equals_plain_double_loops(mode):
    a, cand, t, y, z = ic.class_inputs(5, 9, 11)
    assert mode == ic.ALL or (ic.negatives_mask(t, y, z).sum() < 45 and ic.positives_mask(t, y, z).sum() > 5)   # the masks select something
    tau, inv = st.f32(0.1), st.f32(1.0 / 5)
    want, got = ic.loops64(a, cand, t, y, z, tau, inv, mode), ic.classes64(a, cand, t, y, z, tau, inv, mode)
    for k in want:
        assert np.abs(got[k] - want[k]).max() <= 1e-12 * st.scale(want[k]), k


def test_mode_all_is_the_label_blind_restatement():
    a, cand, t, y, z = ic.class_inputs(5, 65, 3)
    got, want = ic.classes64(a, cand, t, y, z, 0.1, 0.2, ic.ALL), st.inbatch64(a, cand, t, 0.1, 0.2)
    for k in want:
        assert np.abs(got[k] - want[k]).max() <= 1e-9 * st.scale(want[k]), k     # (PD_EPS against the oracle's decimal 1e-6)


@pytest.mark.parametrize("mode, fault", [(ic.OTHER_CLASS, "mask_dropped"), (ic.OTHER_CLASS, "target_masked"),
                                         (ic.MULTI_POSITIVE, "positives_off_by_one")])
def test_planted_faults_are_farther_than_the_yardstick(mode, fault):
    """A restatement that forgets the mask, masks the positive itself, or counts one positive too many is more than 4 D from the
    right one in every output: the bound of the GPU tests tells them apart."""
    B, M, tau, inv = 5, 65, 0.1, 1.0 / 5
    D = ic.classes_distance(B, M, tau, inv, mode)
    a, cand, t, y, z = ic.class_inputs(B, M, 31)
    ref = ic.classes64(a, cand, t, y, z, st.f32(tau), st.f32(inv), mode)
    bad = ic.classes64(a, cand, t, y, z, st.f32(tau), st.f32(inv), mode, fault)
    for k in ref:
        d = float(np.abs(bad[k] - ref[k]).max()) / st.scale(ref[k])
        assert np.isnan(d) or d > 4 * D[k], (k, d, D[k])


@pytest.mark.parametrize("B, M", [(3, 63), (4, 64), (5, 65), (257, 130), (300, 70)])
def test_yardstick_cases_keep_enough_negatives(B, M):
    for s in range(st.SEEDS):
        a, cand, t, y, z = ic.class_inputs(B, M, 7000 + s)
        assert ic.min_negatives(t, y, z) >= ic.MIN_NEGATIVES


# ---- trainer arithmetic on the oracle context ---------------------------------------------------------------------------------
class _LibEx(_Lib):
    """tests/_oracle_ctx.py's entries plus var_inbatch_loss_fwd_bwd_ex, computed by the restatement in fp32."""

    def var_inbatch_loss_fwd_bwd_ex(self, h, s, anchor, cand, target, acls, ccls, B, M, tau, inv, mode, scratch, loss, ga, gc):
        self.calls.append(("inbatch_ex", B, M, inv, mode))
        assert mode in (1, 2) and acls and ccls
        r = ic.classes_torch(_arr(anchor, 3 * B).copy().reshape(B, 3), _arr(cand, 3 * M).copy().reshape(M, 3),
                             _arr(target, B, np.int32).copy(), _arr(acls, B, np.int32).copy(), _arr(ccls, M, np.int32).copy(),
                             tau, inv, mode, torch.float32)
        _arr(loss, 1)[0] = float(r["loss"][0])
        _arr(ga, 3 * B)[:] = r["ga"].reshape(-1)
        _arr(gc, 3 * M)[:] = r["gc"].reshape(-1)
        return 0


class OracleContextEx(OracleContext):
    def __init__(self):
        super().__init__()
        self.lib = _LibEx()


def _cfg(hw=84):
    return types.SimpleNamespace(img_dim=(3, hw, hw), sound_dim=(1, 100, 40), representationDim=3)


def _pool(n_items, seed=3):
    return var_amd.SyntheticTripletPool(n_items, hw=84, seed=seed, clips_per_class=2, device="cpu").freeze_pairs()


def _features(pool, clip_idx, lens):
    out = np.zeros((len(clip_idx), 1, 100, 40), np.float32)
    clips = pool.clips.numpy()
    for i, (c, n) in enumerate(zip(clip_idx.tolist(), lens.tolist())):
        if n > 0:
            out[i] = mfcc_np.process_sound_feat(mfcc_np.mfcc_torchaudio(clips[c, :n], dtype=np.float32))
    return torch.from_numpy(out)


def _batch(B, seed=100):
    g = torch.Generator().manual_seed(seed)
    img = torch.randint(0, 256, (B, 3, 84, 84), dtype=torch.uint8, generator=g)
    snd = torch.randn(2, B, 1, 100, 40, generator=g) * 4
    gt = torch.randint(0, 5, (B,), generator=g).to(torch.int32)
    sn = torch.randint(0, 5, (B,), generator=g).to(torch.int32)
    return img, snd, gt, sn


def _full_batch_reference(sd, img, snd, gt, sn, world, mode, tau=0.1):
    """ONE process scoring every anchor against the candidates [p0 ; n0 ; p1 ; n1 ; ...] with classes ordered alike, torch
    autograd end to end (encoder included): (loss, gradient arena)."""
    net = KukaNetCPU()
    net.load_state_dict(sd)
    Bl = img.shape[0] // world
    a, p, n = net(img.float() / 255., snd[0], snd[1])
    sl = [slice(r * Bl, (r + 1) * Bl) for r in range(world)]
    cand = torch.cat([torch.cat([p[s], n[s]]) for s in sl])
    z = torch.cat([torch.cat([gt[s], sn[s]]) for s in sl]).numpy()
    target = torch.cat([torch.arange(Bl) + r * 2 * Bl for r in range(world)]).numpy()
    loss = ic.classes_loss(a, cand, target, gt.numpy(), z, tau, 1.0 / img.shape[0], mode)
    loss.backward()
    G = torch.cat([dict(net.named_parameters())[k].grad.reshape(-1) for k, _ in var_amd.PARAM_SPECS]).numpy()
    return float(loss.detach()), G


@pytest.mark.parametrize("negatives", ["other_class", "multi_positive"])
def test_eager_step_inbatch_with_classes_equals_the_end_to_end_restatement(negatives):
    torch.manual_seed(5)
    model = var_amd.VARPretextNet(_cfg())
    sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
    ctx = OracleContextEx()
    tr = var_amd.VARTrainer(model, lr=1e-3, _ctx=ctx)
    img, snd, gt, sn = _batch(6)
    assert ic.negatives_mask(np.arange(6), gt.numpy(), torch.cat([gt, sn]).numpy()).sum() < 6 * 12     # something is masked
    tr.step_inbatch(img, snd[0].contiguous(), snd[1].contiguous(), tau=0.1, classes=(gt, sn), negatives=negatives)
    loss, G = _full_batch_reference(sd, img, snd, gt, sn, 1, ic.MODES[negatives])
    assert [c for c in ctx.lib.calls if c[0].startswith("inbatch")] == [("inbatch_ex", 6, 12, 1.0 / 6, ic.MODES[negatives])]
    assert abs(float(tr.loss) - loss) < 2e-6
    assert np.max(np.abs(tr.grads.numpy() - G)) < 1e-5 * max(1.0, np.max(np.abs(G)))


def test_classes_with_negatives_all_is_the_step_without_classes():
    torch.manual_seed(5)
    ma, mb = var_amd.VARPretextNet(_cfg()), var_amd.VARPretextNet(_cfg())
    mb.load_state_dict(ma.state_dict())
    ca, cb = OracleContextEx(), OracleContextEx()
    ta, tb = var_amd.VARTrainer(ma, lr=1e-3, _ctx=ca), var_amd.VARTrainer(mb, lr=1e-3, _ctx=cb)
    img, snd, gt, sn = _batch(4)
    ta.step_inbatch(img, snd[0].contiguous(), snd[1].contiguous(), tau=0.1)
    tb.step_inbatch(img, snd[0].contiguous(), snd[1].contiguous(), tau=0.1, classes=(gt, sn), negatives="all")
    assert ca.lib.calls == cb.lib.calls and ("inbatch", 4, 8, 0.25) in cb.lib.calls      # the old entry, as today
    assert torch.equal(ta.gbuf, tb.gbuf) and torch.equal(ma.flat_parameters(), mb.flat_parameters())


@pytest.mark.parametrize("negatives", ["other_class", "multi_positive"])
def test_replayed_step_with_classes_equals_eager_on_the_same_rows(negatives):
    """capture_inbatch_epoch_steps(classes = the pool's tables) gathers each step's classes by its index row: the same losses and
    parameters as eager step_inbatch calls handed (gt[rows], sn[rows]); the bounds of test_trainer_host.py's label-blind twin."""
    torch.manual_seed(3)
    ma, mb = var_amd.VARPretextNet(_cfg()), var_amd.VARPretextNet(_cfg())
    mb.load_state_dict(ma.state_dict())
    ta = var_amd.VARTrainer(ma, lr=1e-3, _ctx=OracleContextEx())
    cb = OracleContextEx()
    tb = var_amd.VARTrainer(mb, lr=1e-3, _ctx=cb)
    pool = _pool(12)
    gt_tab, sn_tab = pool.class_tables()
    assert gt_tab.dtype == sn_tab.dtype == torch.int32 and gt_tab.is_contiguous() and gt_tab.shape == sn_tab.shape == (12,)
    assert torch.equal(gt_tab.long(), pool.gt) and torch.equal(sn_tab.long(), pool.sn) and int(gt_tab.max()) == pool.task_num
    B = 4
    table = pool.index_table(B, 3, drop_last=True)
    replay, _ = tb.capture_inbatch_epoch_steps(pool.images, pool.clips, B, table, tau=0.1, classes=(gt_tab, sn_tab),
                                               negatives=negatives)
    for s in range(4):                                             # the 4th replay wraps to row 0
        r = table[s % 3]
        rows = r[:B].long()
        want = float(ta.step_inbatch(pool.images[rows].contiguous(), _features(pool, r[B:2 * B], r[3 * B:4 * B]),
                                     _features(pool, r[2 * B:3 * B], r[4 * B:]), tau=0.1,
                                     classes=(gt_tab[rows].contiguous(), sn_tab[rows].contiguous()), negatives=negatives).item())
        got = float(replay().item())
        assert abs(got - want) < 1e-6, (s, got, want)
    assert float((ma.flat_parameters() - mb.flat_parameters()).abs().max()) < 2e-5      # 4 Adam steps of lr 1e-3
    assert [c[4] for c in cb.lib.calls if c[0] == "inbatch_ex"] == [ic.MODES[negatives]] * 4


def test_bad_classes_and_modes_are_refused():
    model = var_amd.VARPretextNet(_cfg())
    tr = var_amd.VARTrainer(model, _ctx=OracleContextEx())
    img, snd, gt, sn = _batch(4)
    pos, neg = snd[0].contiguous(), snd[1].contiguous()
    bad = [dict(negatives="other_class"), dict(negatives="multi_positive"),                  # no classes
           dict(classes=(gt, sn), negatives="same_class"),                                   # no such mode
           dict(classes=(gt[:3].contiguous(), sn), negatives="other_class"),                 # wrong length
           dict(classes=(gt, sn.long()), negatives="other_class"),                           # wrong dtype
           dict(classes=(gt, sn.to("meta")), negatives="multi_positive"),                    # wrong device
           dict(classes=(gt.long(), sn), negatives="all")]                                   # checked even where unused
    for kw in bad:
        with pytest.raises(var_amd.VarHipError):
            tr.step_inbatch(img, pos, neg, **kw)
    pool = _pool(12)
    table = pool.index_table(4, 3, drop_last=True)
    gt_tab, sn_tab = pool.class_tables()
    for kw in (dict(negatives="other_class"), dict(classes=(gt_tab[:4].contiguous(), sn_tab[:4].contiguous()), negatives="other_class"),
               dict(classes=(gt_tab.long(), sn_tab.long()), negatives="multi_positive")):
        with pytest.raises(var_amd.VarHipError):
            tr.capture_inbatch_epoch_steps(pool.images, pool.clips, 4, table, **kw)
    assert tr.step_count == 0


def test_pool_training_loop_with_the_inbatch_head():
    """train_representation_from_pool(head="inbatch") walks the captured in-batch step with the pool's class tables: the same
    per-epoch losses as the replayed step over the same epoch tables; the iTHOR model and ragged epochs are refused."""
    torch.manual_seed(21)
    ma, mb = var_amd.VARPretextNet(_cfg()), var_amd.VARPretextNet(_cfg())
    mb.load_state_dict(ma.state_dict())
    B, epochs = 4, 2
    ctx = OracleContextEx()
    out = var_amd.train_representation_from_pool(ma, _pool(8, seed=5), epochs, B, lr=1e-3, milestones=(1,), gamma=0.5,
                                                 log=lambda *a: None, _ctx=ctx, head="inbatch", tau=0.2, negatives="other_class")
    assert [c[4] for c in ctx.lib.calls if c[0] == "inbatch_ex"] == [ic.OTHER_CLASS] * 4
    pool = _pool(8, seed=5)
    tr = var_amd.VARTrainer(mb, lr=1e-3, _ctx=OracleContextEx())
    want, replay = [], None
    for ep in range(epochs):
        tr.set_lr(var_amd.multistep_lr(1e-3, (1,), 0.5, ep))
        table = pool.epoch_index_table(B)
        if replay is None:
            replay, load = tr.capture_inbatch_epoch_steps(pool.images, pool.clips, B, table, tau=0.2, clip_len=pool.clip_len,
                                                          classes=pool.class_tables(), negatives="other_class")
        else:
            load(table)
        want.append(sum(float(replay().item()) for _ in range(2)) / 2)
    np.testing.assert_allclose(out, want, atol=1e-6)
    assert torch.equal(ma.flat_parameters(), mb.flat_parameters())
    with pytest.raises(var_amd.VarHipError, match="divide"):
        var_amd.train_representation_from_pool(ma, _pool(10), 1, 4, _ctx=OracleContextEx(), head="inbatch")
    with pytest.raises(var_amd.VarHipError, match="head"):
        var_amd.train_representation_from_pool(ma, _pool(8), 1, 4, _ctx=OracleContextEx(), head="softmax")
    with pytest.raises(var_amd.VarHipError, match="triplet"):
        var_amd.train_representation_from_pool(ma, _pool(8), 1, 4, _ctx=OracleContextEx(), negatives="other_class")
    ithor = var_amd.IthorVARPretextNet(types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 600, 40), representationDim=3))
    with pytest.raises(var_amd.VarHipError, match="iTHOR"):
        var_amd.train_representation_from_pool(ithor, _pool(8), 1, 4, head="inbatch")


# ---- two gloo ranks ----------------------------------------------------------------------------------------------------------
def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _worker(rank, world, port, out, negatives):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    torch.set_num_threads(2)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(5)
    model = var_amd.VARPretextNet(_cfg())
    tr = var_amd.VARTrainer(model, lr=1e-3, _ctx=OracleContextEx())
    Bl = 3
    img, snd, gt, sn = _batch(world * Bl)
    sl = slice(rank * Bl, (rank + 1) * Bl)
    tr.step_inbatch(img[sl].contiguous(), snd[0, sl].contiguous(), snd[1, sl].contiguous(), tau=0.1,
                    classes=(gt[sl].contiguous(), sn[sl].contiguous()), negatives=negatives)
    out.put((rank, tr.gbuf.numpy().copy(), model.flat_parameters().numpy().copy()))
    dist.destroy_process_group()


@pytest.mark.parametrize("negatives", ["other_class", "multi_positive"])
def test_two_ranks_with_classes_equal_the_full_batch_restatement(negatives):
    """2 ranks x 3 triplets (the classes all-gathered beside the embeddings, anchors' classes = the rank's own gt) against ONE
    process scoring 6 anchors on 12 candidates with classes, as tests/test_dp_gloo.py does for the label-blind head."""
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q, negatives)) for r in range(2)]
    for p in procs:
        p.start()
    got = sorted([q.get(timeout=600) for _ in range(2)], key=lambda t: t[0])
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    torch.manual_seed(5)
    sd = {k: v.detach().clone() for k, v in var_amd.VARPretextNet(_cfg()).state_dict().items()}
    img, snd, gt, sn = _batch(6)
    loss, G = _full_batch_reference(sd, img, snd, gt, sn, 2, ic.MODES[negatives])
    blind, _ = _full_batch_reference(sd, img, snd, gt, sn, 2, ic.ALL)
    assert abs(loss - blind) > 1e-3                                   # the classes matter at this draw
    for _rank, buf, _flat in got:
        assert abs(buf[-1] - loss) < 2e-6
        assert np.max(np.abs(buf[:-1] - G)) < 1e-5 * max(1.0, np.max(np.abs(G)))
    assert np.array_equal(got[0][2], got[1][2])

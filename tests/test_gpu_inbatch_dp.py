"""Two REAL ranks on the in-batch step of both trainers (-m gpu): both processes drive the HIP library on cuda:0 and exchange through
gloo, as tests/test_gpu_dp2.py does it (RCCL refuses two ranks on one device).  What runs here and nowhere else on real kernels:
the multi-rank branch of VARTrainer.capture_inbatch_epoch_steps (four graphs, three eager collectives, the static cand / ccls
buffers, allgather(out=), the rank offset lo = rank * 2B in captured pointers, the classes gathered again on every replay) and
IthorTrainer.step_inbatch with more than one rank.  One spawn per trainer: a worker walks the three treatments of an anchor's own
class itself (tests/_inbatch_dp.py ends the test at once when a rank fails).  Three layers per step:
  1. the exchange, bit for bit: cand = [local_0 ; local_1] and ccls = [gt_0 ; sn_0 ; gt_1 ; sn_1] on both ranks, the reduced candidate
     gradients, [gradients | loss] and the parameters equal on both ranks, the loss slot = fp32(loss_0 + loss_1);
  2. the head against the float64 restatement of tests/inbatch_classes_cpu.py on what was gathered, target = arange(B) + lo_r, inv_count
     = 1 / (2B): each rank's loss and anchor gradients, the summed candidate gradients, within four times torch fp32's own distance
     from float64 at the same case, the rule tests/test_gpu_inbatch_classes.py holds the head to.  Its classes_distance measures that
     over 20 draws of unit vectors and refuses M = 12 and M = 8 (a draw leaves a row fewer than 8 negatives); here the draws are
     what the steps themselves gathered -- embeddings of a fresh model lie close together, where a_i - c_j cancels and fp32 is
     farther from float64 than on unit vectors -- and the distance is the largest over the steps and ranks of a trainer and mode;
  3. the step against ONE process on the global batch in the ranks' candidate order [p0 ; n0 ; p1 ; n1]: the Kuka step at
     tests/test_gpu_dp2.py's tolerances (losses atol 1e-5, parameters max < 1e-4 and 99 % within 2e-6); the iTHOR arena against the
     float64 sum of two one-process half-batch arenas, within MARGIN = 4 times the distance of the whole-batch arena from that sum
     (the embeddings of batch 2 against batch 4 have no project bound, so it is measured here, on the same kernels).
No bound here was taken from what the two-rank code gives.
Seen on an MI355X (DESIGN section 6 has the table): the head at 0.27 .. 0.47 of its bounds (g_anchor 1.0e-5 .. 2.3e-5 of its largest
magnitude against bounds of 3.9e-5 .. 7.6e-5); Kuka against one process: losses within 7.2e-7, parameters within 1.1e-5; iTHOR: the
whole batch 1.6e-7 .. 4.7e-7 from the sum of the halves, the two ranks 1.9e-8 .. 4.0e-8 from it."""
import hashlib
import os
import types

import numpy as np
import pytest
import torch

from tests import inbatch_classes_cpu as ic
from tests import step_tail_cpu as st
from tests._inbatch_dp import ITEMS, NAMES, Ranks, assert_classes_differ, candidate_classes, init_group, rank_items, report
from tests.test_gpu_dp2 import _cfg, _tables

pytestmark = pytest.mark.gpu

MARGIN = 4
TAU = 0.1


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def _host(t):
    return t.detach().cpu().numpy().copy()


def _digest(t):
    return hashlib.sha256(_host(t).tobytes()).hexdigest()


def _start(rank, world, port):
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    init_group(rank, world, port)


def check_exchange(a, b, B, zs, mode, where):
    """Layer 1 on the snapshots a, b of ranks 0 and 1 after one step."""
    cand = np.concatenate([a["emb"][1:].reshape(2 * B, 3), b["emb"][1:].reshape(2 * B, 3)])
    for r, x in enumerate((a, b)):
        assert np.array_equal(x["cand"].view(np.uint32), cand.view(np.uint32)), where
        assert np.array_equal(x["target"], np.arange(B) + 2 * B * r), where
        if mode:
            assert np.array_equal(x["ccls"], zs), (where, r, x["ccls"], zs)
    assert np.array_equal(a["gc"], b["gc"]), where                                    # (a two-rank sum is one commutative fp32 add)
    assert np.isfinite(a["gc"]).all() and np.abs(a["gc"]).max() > 0, where
    return cand


def check_heads(cases, B, mode):
    """Layer 2 over the steps of one trainer in one mode, cases = [(a, b, cand, ys, zs, where)]: the head's outputs against the float64
    restatement, within MARGIN times torch fp32's own distance from it -- per output the largest over these steps and ranks, as
    classes_distance takes the largest over its draws.  Returns the largest distance / bound."""
    tau, inv = st.f32(TAU), st.f32(1.0 / (2 * B))
    dist = lambda x, ref: float(np.abs(np.asarray(x, np.float64).reshape(ref.shape) - ref).max()) / st.scale(ref)      # noqa: E731
    D, seen = {"loss": 0.0, "ga": 0.0, "gc": 0.0}, []
    for a, b, cand, ys, zs, where in cases:
        args = [(x["emb"][0], cand, x["target"].astype(np.int32), ys[r], zs, tau, inv, mode) for r, x in enumerate((a, b))]
        refs, t32 = [ic.classes64(*q) for q in args], [ic.classes_torch(*q, torch.float32) for q in args]
        gc = refs[0]["gc"] + refs[1]["gc"]
        for r, x in enumerate((a, b)):
            for k in ("loss", "ga"):
                D[k] = max(D[k], dist(t32[r][k], refs[r][k]))
                seen.append((k, dist(x[k], refs[r][k]), f"{where} rank {r}"))
        D["gc"] = max(D["gc"], dist(t32[0]["gc"] + t32[1]["gc"], gc))                     # (one fp32 add, as the all-reduce's)
        seen.append(("gc", dist(a["gc"], gc), where))
        total = np.float32(a["loss"][0]) + np.float32(b["loss"][0])                        # the loss slot after the arena's all-reduce
        for x in (a, b):
            assert np.float32(x["arena_loss"]) == total, (where, x["arena_loss"], total)
    worst = {k: max(d for kk, d, _ in seen if kk == k) for k in D}
    print(f"head, mode {mode}, {len(cases)} steps: " + " ".join(f"{k} {worst[k]:.2e}/{MARGIN * D[k]:.2e}" for k in D))
    for k, d, where in seen:
        assert d <= MARGIN * D[k], (where, k, d, MARGIN * D[k])
    return max(worst[k] / (MARGIN * D[k]) for k in D)


# ---- the Kuka trainer, captured ------------------------------------------------------------------------------------------------
KUKA_B, KUKA_REPLAYS = 3, 3


def _kuka_kw(negatives, gt, sn):
    return {} if negatives == "all" else dict(classes=(gt, sn), negatives=negatives)


def _kuka_rank(rank, world, port):
    import var_amd
    _start(rank, world, port)
    B = KUKA_B
    pool = var_amd.SyntheticTripletPool(12, hw=84, seed=3, clips_per_class=4).freeze_pairs()
    gt_tab, sn_tab = pool.class_tables()
    table = _tables(pool, world, B, ITEMS)[rank]
    out = {}
    for negatives in NAMES:
        torch.manual_seed(7 + rank)                              # different initial weights: the trainer broadcasts rank 0's
        model = var_amd.VARPretextNet(_cfg()).to("cuda")
        tr = var_amd.VARTrainer(model, lr=1e-3)
        replay, _ = tr.capture_inbatch_epoch_steps(pool.images, pool.clips, B, table, tau=TAU, **_kuka_kw(negatives, gt_tab, sn_tab))
        _img, _feats, emb, cand, target, lcls, ccls, _scratch, loss, ga, gc = tr._keep_inbatch
        steps = [dict(params=_host(model.flat_parameters()))]
        for _ in range(KUKA_REPLAYS):
            arena_loss = float(replay().item())
            steps.append(dict(emb=_host(emb), cand=_host(cand), target=_host(target), lcls=_host(lcls), ccls=_host(ccls), loss=_host(loss),
                              ga=_host(ga), gc=_host(gc), gbuf=_host(tr.gbuf), params=_host(model.flat_parameters()), arena_loss=arena_loss))
        out[negatives] = (steps, tr.step_count)
    return out


def _kuka_worker(rank, world, port, out):
    report(out, rank, _kuka_rank, rank, world, port)


def _one_process_step(var_amd, tr, pool, items, negatives):
    """ONE process scoring the global row's anchors on [p0 ; n0 ; p1 ; n1] and stepping, as tests/test_gpu_inbatch_classes.py's two-rank
    test builds it, for any treatment of the classes: (loss, label-blind loss)."""
    from var_amd._lib import ptr
    model, c = tr.model, tr.ctx
    n = len(items) // 2
    i = torch.tensor(items, device="cuda")
    gt_tab, sn_tab = pool.class_tables()
    f = var_amd.mfcc(pool.clips, pool.len_tab[:, i].reshape(-1), 100, pool.clip_tab[:, i].reshape(-1))
    pos, neg = f[:2 * n], f[2 * n:]
    img = pool.images[i].contiguous()
    emb = torch.empty((3, 2 * n, 3), device="cuda")
    tr._bind()
    c.ensure_plan(2 * n, 84)
    c.check(c.lib.var_arm_encoder_fwd(c.handle, c.stream(), ptr(model.flat_parameters()), ptr(img), 1, img.stride(0), ptr(pos), ptr(neg),
                                      2 * n, 84, ptr(emb[0]), ptr(emb[1]), ptr(emb[2]), None, None, 1), "fwd")
    cand = torch.cat([emb[1, :n], emb[2, :n], emb[1, n:], emb[2, n:]]).contiguous()
    target = torch.cat([torch.arange(n), torch.arange(n) + 2 * n]).to(torch.int32).cuda()
    kw = {} if negatives == "all" else dict(anchor_cls=gt_tab[i].contiguous(), cand_cls=candidate_classes(gt_tab, sn_tab, items).contiguous(),
                                            negatives=negatives)
    loss, ga, gc = var_amd.inbatch_contrastive_loss(emb[0], cand, target, tau=TAU, **kw)
    blind = float(var_amd.inbatch_contrastive_loss(emb[0], cand, target, tau=TAU)[0].item())
    gp = torch.cat([gc[:n], gc[2 * n:3 * n]]).contiguous()
    gn = torch.cat([gc[n:2 * n], gc[3 * n:]]).contiguous()
    c.check(c.lib.var_arm_encoder_bwd(c.handle, c.stream(), ptr(model.flat_parameters()), ptr(ga), ptr(gp), ptr(gn), ptr(tr.gbuf)), "bwd")
    tr.gbuf[var_amd.N_PARAMS:].copy_(loss)
    tr.adam()
    return float(loss.item()), blind


def test_kuka_captured_step_on_two_ranks(var_amd):
    """B_local = 3 (2B = 6, M = 12: rank 1's rows start at lo = 6, no multiple of the 4 rows a head workgroup takes), two index rows,
    three replays per mode (the third wraps to row 0).  The one process needs nothing of the ranks and steps while they start."""
    B = KUKA_B
    with Ranks(_kuka_worker) as ranks:
        pool = var_amd.SyntheticTripletPool(12, hw=84, seed=3, clips_per_class=4).freeze_pairs()
        one = {}
        for negatives in NAMES:
            torch.manual_seed(7)
            model = var_amd.VARPretextNet(_cfg()).to("cuda")
            tr = var_amd.VARTrainer(model, lr=1e-3)
            start = _host(model.flat_parameters())
            steps = [_one_process_step(var_amd, tr, pool, ITEMS[s % 2], negatives) for s in range(KUKA_REPLAYS)]
            one[negatives] = (start, [w for w, _ in steps], [bl for _, bl in steps], _host(model.flat_parameters()))
        got = ranks.collect()
    gt_tab, sn_tab = (t.cpu() for t in pool.class_tables())
    assert_classes_differ(gt_tab, sn_tab)
    for negatives in NAMES:
        mode = ic.MODES[negatives]
        (r0, n0), (r1, n1) = got[0][negatives], got[1][negatives]
        assert n0 == n1 == KUKA_REPLAYS
        start, want, blind, params = one[negatives]
        assert np.array_equal(r0[0]["params"], r1[0]["params"]) and np.array_equal(r0[0]["params"], start)      # the broadcast
        cases = []
        for s in range(KUKA_REPLAYS):
            items = ITEMS[s % 2]
            where = f"kuka {negatives} replay {s}"
            a, b = r0[s + 1], r1[s + 1]
            zs = candidate_classes(gt_tab, sn_tab, items).numpy()
            ys = [gt_tab[rank_items(items, r)].numpy().astype(np.int32) for r in range(2)]
            if mode:                                             # the rank's own [gt ; sn], gathered by the captured forward
                assert all(np.array_equal(x["lcls"], zs[2 * B * r:2 * B * (r + 1)]) for r, x in enumerate((a, b))), where
            cand = check_exchange(a, b, B, zs, mode, where)
            assert np.array_equal(a["gbuf"], b["gbuf"]) and np.array_equal(a["params"], b["params"]), where
            assert not np.array_equal(a["params"], r0[s]["params"]), where
            cases.append((a, b, cand, ys, zs, where))
        head = check_heads(cases, B, mode)
        losses = [x["arena_loss"] for x in r0[1:]]
        assert mode == ic.ALL or max(abs(w - x) for w, x in zip(want, blind)) > 1e-3       # the classes matter on these rows
        np.testing.assert_allclose(losses, want, atol=1e-5)
        d = np.abs(r0[-1]["params"] - params)
        print(f"kuka {negatives}: head at {head:.2f} of its bound; against one process: loss {max(abs(x - w) for x, w in zip(losses, want)):.2e}, "
              f"parameters max {d.max():.2e}, within 2e-6: {np.mean(d < 2e-6):.4f}")
        assert d.max() < 1e-4 and np.mean(d < 2e-6) > 0.99, (d.max(), np.mean(d < 2e-6))


# ---- the iTHOR trainer, eager --------------------------------------------------------------------------------------------------
ITHOR_B, ITHOR_STEPS = 2, 2
# global batches of 4, rank r takes rows [2r, 2r + 2): rank 1's anchors (classes 1 0, then 0 4) meet their classes among rank 0's
# candidates ([gt ; sn] = 0 1 1 4, then 4 0 0 1); a negative never has its anchor's class (dataset.py:70-78)
ITHOR_GT = ((0, 1, 1, 0), (4, 0, 0, 4))
ITHOR_SN = ((1, 4, 0, 4), (0, 1, 4, 1))


def _ithor_cfg():
    return types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 600, 40), representationDim=3)


def _ithor_inputs():
    """Drawn as tests/test_gpu_inbatch_step.py draws them, at the global batch of 4, once per step."""
    g = torch.Generator().manual_seed(9 + 2 * ITHOR_B)
    steps = []
    for s in range(ITHOR_STEPS):
        img = torch.randint(0, 256, (2 * ITHOR_B, 3, 96, 96), dtype=torch.uint8, generator=g)
        pos, neg = (torch.randn(2 * ITHOR_B, 1, 600, 40, generator=g) * 4 for _ in range(2))
        steps.append((img, pos, neg, torch.tensor(ITHOR_GT[s], dtype=torch.int32), torch.tensor(ITHOR_SN[s], dtype=torch.int32)))
    return steps


def _ithor_kw(negatives, gt, sn):
    return {} if negatives == "all" else dict(classes=(gt.cuda().contiguous(), sn.cuda().contiguous()), negatives=negatives)


def _ithor_rank(rank, world, port):
    import var_amd
    import var_amd.ithor as ithor
    from var_amd.inbatch import InbatchStep
    _start(rank, world, port)
    taken = []

    class Snapshot(InbatchStep):                                 # the product's step, looked at after its last phase
        def run(self, *a, **k):
            super().run(*a, **k)
            loss, ga, gc = self.out
            taken.append(dict(emb=_host(self.emb), cand=_host(self.cand), target=_host(self.target), loss=_host(loss), ga=_host(ga),
                              gc=_host(gc), ccls=None if self.ccls is None else _host(self.ccls)))

    ithor.InbatchStep = Snapshot
    B, sl = ITHOR_B, slice(rank * ITHOR_B, (rank + 1) * ITHOR_B)
    out = {}
    torch.manual_seed(123)                                       # (IthorTrainer broadcasts nothing: the replicas start from one seed)
    m = var_amd.IthorVARPretextNet(_ithor_cfg()).to("cuda")
    start = m.flat_parameters().clone()
    for negatives in NAMES:
        m.flat_parameters().copy_(start)
        tr = var_amd.IthorTrainer(m, lr=1e-4)
        assert tr.world == world and tr.rank == rank
        steps = []
        for img, pos, neg, gt, sn in _ithor_inputs():
            arena_loss = float(tr.step_inbatch(img[sl].cuda(), pos[sl].cuda(), neg[sl].cuda(), tau=TAU, **_ithor_kw(negatives, gt[sl], sn[sl])).item())
            snap = taken.pop()
            assert not taken and snap["emb"].shape == (3, B, 3)
            snap.update(arena_loss=arena_loss, gbuf_digest=_digest(tr.gbuf), params_digest=_digest(m.flat_parameters()),
                        gbuf=_host(tr.gbuf) if rank == 0 else None)       # (15 MB: one copy travels, the other rank's as its digest)
            steps.append(snap)
        out[negatives] = (steps, tr.step_count)
    return out


def _ithor_worker(rank, world, port, out):
    report(out, rank, _ithor_rank, rank, world, port)


def _ithor_arena(m, img, pos, neg, grads=None):
    """_IthorFn forward on the rows given; grads = (ga, gp, gn) or a function of the embeddings that gives them: backward too.
    Returns (embeddings (3, B, 3) detached, arena or None)."""
    m.zero_grad(set_to_none=True)
    d = m(img, pos, neg)
    emb = [d[k] for k in ("image_feat", "sound_feat_positive", "sound_feat_negative")]
    det = torch.stack([e.detach() for e in emb]).contiguous()
    if grads is None:
        return det, None
    torch.autograd.backward(emb, list(grads(det) if callable(grads) else grads))
    return det, torch.cat([p.grad.reshape(-1) for p in m.parameters()]).clone()


def _ithor_reference(var_amd, m, step, negatives):
    """ONE process on a global batch from the model's present parameters: the whole batch in the ranks' candidate order (forward on
    all 4 rows, head, backward), and the two half-batches through the same kernels -- forward both, the head per half on all
    candidates, one fp32 sum of the candidate gradients, backward per half -- their arenas and losses added in float64.
    D: the distance of the whole batch's arena from that sum, relative to max |G|."""
    B = ITHOR_B
    img, pos, neg, gt, sn = step
    img, pos, neg, gt = img.cuda(), pos.cuda(), neg.cuda(), gt.cuda()
    zs = torch.cat([gt[:B], sn[:B].cuda(), gt[B:], sn[B:].cuda()]).contiguous()
    kw = (lambda y: {}) if negatives == "all" else (lambda y: dict(anchor_cls=y.contiguous(), cand_cls=zs, negatives=negatives))
    whole = {}

    def whole_head(emb):
        target = torch.cat([torch.arange(B), torch.arange(B) + 2 * B]).to(torch.int32).cuda()
        cand = torch.cat([emb[1, :B], emb[2, :B], emb[1, B:], emb[2, B:]]).contiguous()              # [p0 ; n0 ; p1 ; n1]
        whole["loss"], ga, gc = var_amd.inbatch_contrastive_loss(emb[0], cand, target, TAU, 1.0 / (2 * B), **kw(gt))
        return ga, torch.cat([gc[:B], gc[2 * B:3 * B]]).contiguous(), torch.cat([gc[B:2 * B], gc[3 * B:]]).contiguous()
    G = _ithor_arena(m, img, pos, neg, whole_head)[1].double().cpu().numpy()
    halves = [slice(0, B), slice(B, 2 * B)]
    embs = [_ithor_arena(m, img[h], pos[h], neg[h])[0] for h in halves]
    cand = torch.cat([e[1:].reshape(2 * B, 3) for e in embs]).contiguous()
    outs = [var_amd.inbatch_contrastive_loss(embs[r][0], cand, torch.arange(B, dtype=torch.int32, device="cuda") + 2 * B * r, TAU,
                                             1.0 / (2 * B), **kw(gt[h])) for r, h in enumerate(halves)]
    gc = outs[0][2] + outs[1][2]
    S = 0.0
    for r, h in enumerate(halves):                               # (a forward again in front of each backward: the workspace holds one)
        mine = gc[2 * B * r:2 * B * (r + 1)]
        S = S + _ithor_arena(m, img[h], pos[h], neg[h], (outs[r][1], mine[:B].contiguous(), mine[B:].contiguous()))[1].double().cpu().numpy()
    top = float(np.abs(G).max())
    return dict(S=S, top=top, D=float(np.abs(G - S).max()) / top, whole_loss=float(whole["loss"].item()),
                halves_loss=float(outs[0][0].double().item() + outs[1][0].double().item()))


def test_ithor_step_inbatch_on_two_ranks(var_amd):
    """fp32, (3, 96, 96), B_local = 2: M = 8 and lo = 4 on rank 1; two steps per mode on fresh inputs and classes.  The one-process
    reference of the first step needs nothing of the ranks and is computed while they start."""
    B = ITHOR_B
    inputs = _ithor_inputs()
    for s in range(ITHOR_STEPS):
        gt, sn = ITHOR_GT[s], ITHOR_SN[s]
        assert all(g != n for g, n in zip(gt, sn)) and all(y in gt[:B] + sn[:B] for y in gt[B:])
    with Ranks(_ithor_worker) as ranks:
        torch.manual_seed(123)
        m = var_amd.IthorVARPretextNet(_ithor_cfg()).to("cuda")
        start = m.flat_parameters().clone()
        first = {negatives: _ithor_reference(var_amd, m, inputs[0], negatives) for negatives in NAMES}
        got = ranks.collect()
    for negatives in NAMES:
        mode = ic.MODES[negatives]
        (r0, n0), (r1, n1) = got[0][negatives], got[1][negatives]
        assert n0 == n1 == ITHOR_STEPS                           # the device-side step count, on both ranks
        m.flat_parameters().copy_(start)
        tr = var_amd.IthorTrainer(m, lr=1e-4)
        cases = []
        for s, (_img, _pos, _neg, gt, sn) in enumerate(inputs):
            where = f"ithor {negatives} step {s}"
            a, b = r0[s], r1[s]
            zs = torch.cat([gt[:B], sn[:B], gt[B:], sn[B:]]).numpy()
            cand = check_exchange(a, b, B, zs, mode, where)
            assert a["gbuf_digest"] == b["gbuf_digest"] and a["params_digest"] == b["params_digest"], where
            assert np.float32(a["gbuf"][-1]) == np.float32(a["arena_loss"]), where
            cases.append((a, b, cand, [gt[:B].numpy(), gt[B:].numpy()], zs, where))
            # layer 3: one process, from the parameters this step started from
            ref = first[negatives] if s == 0 else _ithor_reference(var_amd, m, inputs[s], negatives)
            d = float(np.abs(a["gbuf"][:-1].astype(np.float64) - ref["S"]).max()) / ref["top"]
            d_halves, d_whole = abs(a["arena_loss"] - ref["halves_loss"]), abs(a["arena_loss"] - ref["whole_loss"])
            print(f"{where}: whole batch from the sum of the halves D = {ref['D']:.2e}, two ranks from it {d:.2e} (bound {MARGIN * ref['D']:.2e}); "
                  f"max |G| {ref['top']:.2e}; loss from the halves' {d_halves:.2e}, from the whole batch's {d_whole:.2e}")
            assert ref["top"] > 0 and d <= MARGIN * ref["D"], (where, d, ref["D"])
            assert d_whole <= 1e-5, (where, d_whole)             # (tests/test_gpu_dp2.py's tolerance of a two-rank loss)
            # the replicas' optimiser step, done again here on their arena: the same kernel on the same bits
            tr.gbuf.copy_(torch.from_numpy(a["gbuf"]))
            tr.adam()
            assert _digest(m.flat_parameters()) == a["params_digest"], where
        assert tr.step_count == ITHOR_STEPS
        print(f"ithor {negatives}: head at {check_heads(cases, B, mode):.2f} of its bound")

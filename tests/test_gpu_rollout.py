"""GPU checks of the PPO rollout around the networks (csrc/rollout.hip: var_rollout_move, var_rollout_returns, var_ppo_head;
var_amd.RolloutStorage / ppo_loss / PPO) against the fixture made from the reference (tests/golden/rollout_t7.npz) and the
restatement of tests/rollout_cpu.py.

Bounds.  Returns: bit for bit.  Copies: bit for bit, neighbours untouched.  Advantages, losses and gradients: four times the
distance of torch's own fp32 evaluation of the same formulas (CPU, autograd for the gradients) from float64 -- the largest
over 20 seeded draws at the tested shape, per output array (rollout_cpu.advantage_distance / loss_distance): a fixed-order
sum or a device expf may round differently from torch's, it may not be worse in kind.  The loss head's distances are relative
to each array's largest magnitude (rollout_cpu.loss_distance says why); the advantages are normalised, theirs are absolute."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import rollout_cpu as rc

pytestmark = pytest.mark.gpu

MODES = {"gae_proper": (True, True), "gae_free": (True, False), "plain_proper": (False, True), "plain_free": (False, False)}
GEN_SEED = 11
SENT = -77.0


class Discrete:
    def __init__(self, n=4):
        self.n = n


class Box:
    def __init__(self, n=2):
        self.shape = (n,)


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


@pytest.fixture(scope="module")
def ctx(var_amd):
    from var_amd._lib import Context
    return Context.get(0)


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "rollout_t7.npz"))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---- returns and advantages -------------------------------------------------------------------------------------------------
def call_returns(ctx, d, gae, proper, want_adv=True):
    T, N = d["rewards"].shape[:2]
    t = {k: dev(v) for k, v in d.items()}
    ret = torch.full((T + 1, N, 1), SENT, device="cuda")
    adv = torch.full((T, N, 1), SENT, device="cuda") if want_adv else None
    rcode = ctx.lib.var_rollout_returns(ctx.handle, None, p(t["rewards"]), p(t["value_preds"]), p(t["masks"]), p(t["bad_masks"]),
                                        p(t["next_value"]), T, N, int(gae), rc.GAMMA, rc.LAMBDA, int(proper), p(ret), p(adv))
    return rcode, ret, t["value_preds"], adv


@pytest.mark.parametrize("mode", sorted(MODES))
def test_returns_equal_the_reference_fixture_bit_for_bit(var_amd, gold, mode):
    """Through RolloutStorage: the fixture's steps go in with insert(), compute_returns() leaves the reference's bits."""
    ro = fixture_storage(var_amd, gold)
    gae, proper = MODES[mode]
    ro.compute_returns(dev(gold["in.next_value"]), gae, rc.GAMMA, rc.LAMBDA, proper)
    assert np.array_equal(bits(host(ro.returns)), bits(gold["ret." + mode]))
    assert np.array_equal(bits(host(ro.value_preds)), bits(gold["vp." + mode]))
    if mode == "gae_proper":
        a64 = rc.advantages64(gold["ret." + mode], gold["vp." + mode])
        d, bound = np.abs(host(ro.advantages()) - a64).max(), 4 * rc.advantage_distance(7, 5)
        print("advantages vs float64:", d, "bound", bound)
        assert d <= bound


@pytest.mark.parametrize("mode", sorted(MODES))
@pytest.mark.parametrize("T, N", [(1, 1), (2, 1), (7, 5), (3, 300), (100, 8)])
def test_returns_and_advantages_at_the_edge_shapes(ctx, T, N, mode):
    gae, proper = MODES[mode]
    d = rc.rollout_inputs(T, N, 31 * T + N)
    assert d["masks"][T, 0, 0] == 0.0 and d["masks"][1, N - 1, 0] == 0.0
    ref_ret, ref_v = rc.compute_returns(d["rewards"], d["value_preds"], d["masks"], d["bad_masks"], d["next_value"], gae, rc.GAMMA,
                                        rc.LAMBDA, proper)
    want_adv = T * N >= 2
    rcode, ret, v, adv = call_returns(ctx, d, gae, proper, want_adv)
    assert rcode == 0
    got_ret = host(ret)
    if gae:                                                      # GAE leaves returns[T] alone, as the reference does
        assert (got_ret[T] == SENT).all()
        got_ret[T] = ref_ret[T]
    assert np.array_equal(bits(got_ret), bits(ref_ret)) and np.array_equal(bits(host(v)), bits(ref_v))
    if not want_adv:
        rcode, ret, v, adv = call_returns(ctx, d, gae, proper, True)        # one value has no standard deviation
        assert rcode == -1
        torch.cuda.synchronize()
        assert (ret == SENT).all() and (adv == SENT).all() and np.array_equal(host(v), d["value_preds"])
        return
    a64 = rc.advantages64(ref_ret, ref_v)
    got = host(adv)
    # torch fp32's own distance from float64: on these inputs, and the largest over 20 more draws at this shape and mode
    dist, bound = np.abs(got - a64).max(), 4 * max(rc.advantage_error32(ref_ret, ref_v), rc.advantage_distance(T, N, gae, proper))
    print(f"(T,N)=({T},{N}) {mode} advantages vs float64: {dist:.3e}, torch fp32's own distance {bound / 4:.3e}")
    assert dist <= bound
    _, _, _, adv2 = call_returns(ctx, d, gae, proper, True)
    assert np.array_equal(bits(host(adv2)), bits(got))                       # the same input: the same bits


def test_returns_refuse_bad_arguments(ctx, var_amd):
    d = rc.rollout_inputs(3, 2, 1)
    t = {k: dev(v) for k, v in d.items()}
    ret = torch.full((4, 2, 1), SENT, device="cuda")
    args = lambda **o: [o.get("r", p(t["rewards"])), p(t["value_preds"]), p(t["masks"]), o.get("bm", p(t["bad_masks"])),      # noqa: E731
                        p(t["next_value"]), o.get("T", 3), o.get("N", 2), 1, 0.99, 0.95, o.get("proper", 1), o.get("ret", p(ret)), None]
    for name, o in (("T", dict(T=0)), ("N", dict(N=0)), ("rewards NULL", dict(r=None)), ("bad_masks NULL", dict(bm=None)),
                    ("returns is value_preds", dict(ret=p(t["value_preds"])))):
        assert ctx.lib.var_rollout_returns(ctx.handle, None, *args(**o)) == -1, name
    torch.cuda.synchronize()
    assert (ret == SENT).all()
    assert ctx.lib.var_rollout_returns(ctx.handle, None, *args(bm=None, proper=0)) == 0


# ---- the move kernel --------------------------------------------------------------------------------------------------------
OBS_SHAPES = {'image': (3, 96, 96), 'flag': (1,), 'pose': (3,), 'cell': (2,), 'gain': (1,)}
OBS_DTYPES = {'image': torch.uint8, 'flag': torch.uint8, 'pose': torch.float32, 'cell': torch.int64, 'gain': torch.float32}


def random_like(t, g):
    if t.dtype == torch.uint8:
        return torch.randint(0, 256, t.shape, dtype=torch.uint8, generator=g).cuda()
    if t.dtype == torch.int64:
        return torch.randint(-2 ** 40, 2 ** 40, t.shape, dtype=torch.int64, generator=g).cuda()
    return torch.randn(t.shape, generator=g).cuda()


def all_stores(ro):
    s = {"obs." + k: v for k, v in ro.obs.items()} if isinstance(ro.obs, dict) else {"obs": ro.obs}
    s.update(hxs=ro.recurrent_hidden_states, actions=ro.actions, logp=ro.action_log_probs, value_preds=ro.value_preds,
             rewards=ro.rewards, masks=ro.masks, bad_masks=ro.bad_masks)
    return s


@pytest.mark.parametrize("space", [Discrete(4), Box(2)])
def test_insert_and_after_update_equal_copy_(var_amd, space):
    """Rows of 27648 (u8 image), 1, 12, 16 and 4 bytes beside the fixed members, every step index including the wrap; the
    mirror does storage.py:61-87 with copy_.  Comparing whole tensors also shows that no other slot was touched."""
    T, N = 3, 3
    cfg = types.SimpleNamespace(RLObsIgnore=['debug'])
    ro = var_amd.RolloutStorage(T, N, {**OBS_SHAPES, 'debug': (5,)}, space, 20, cfg, image_dtype=OBS_DTYPES)
    assert 'debug' not in ro.obs and ro.obs['image'].dtype == torch.uint8 and ro.obs['image'].shape == (T + 1, N, 3, 96, 96)
    assert ro.actions.dtype == (torch.int64 if isinstance(space, Discrete) else torch.float32)
    g = torch.Generator().manual_seed(5)
    for x in all_stores(ro).values():
        x.copy_(random_like(x, g))                               # every slot recognisable
    mirror = {k: v.clone() for k, v in all_stores(ro).items()}
    step = 0
    for i in range(T + 1):                                       # the fourth insert wraps to step 0
        obs = {k: random_like(ro.obs[k][0], g) for k in OBS_SHAPES}
        feed = dict(hxs=random_like(ro.recurrent_hidden_states[0], g), actions=random_like(ro.actions[0], g),
                    logp=random_like(ro.action_log_probs[0], g), value_preds=random_like(ro.value_preds[0], g),
                    rewards=random_like(ro.rewards[0], g), masks=random_like(ro.masks[0], g), bad_masks=random_like(ro.bad_masks[0], g))
        ro.insert(obs, feed["hxs"], feed["actions"], feed["logp"], feed["value_preds"], feed["rewards"], feed["masks"], feed["bad_masks"])
        for k in OBS_SHAPES:
            mirror["obs." + k][step + 1].copy_(obs[k])
        for k in ("hxs", "masks", "bad_masks"):
            mirror[k][step + 1].copy_(feed[k])
        for k in ("actions", "logp", "value_preds", "rewards"):
            mirror[k][step].copy_(feed[k])
        step = (step + 1) % T
        assert ro.step == step
        torch.cuda.synchronize()
        for k, v in all_stores(ro).items():
            assert torch.equal(v, mirror[k]), (i, k)
    ro.after_update()
    for k in list(OBS_SHAPES) + ["hxs", "masks", "bad_masks"]:
        key = "obs." + k if k in OBS_SHAPES else k
        mirror[key][0].copy_(mirror[key][-1])
    torch.cuda.synchronize()
    for k, v in all_stores(ro).items():
        assert torch.equal(v, mirror[k]), k
    with pytest.raises(var_amd.VarHipError):
        ro.insert({k: v.cpu() for k, v in obs.items()}, *[feed[k] for k in ("hxs", "actions", "logp", "value_preds", "rewards", "masks", "bad_masks")])
    with pytest.raises(var_amd.VarHipError):
        ro.insert({**obs, 'image': obs['image'].float()}, *[feed[k] for k in ("hxs", "actions", "logp", "value_preds", "rewards", "masks", "bad_masks")])
    with pytest.raises(NotImplementedError):
        ro.feed_forward_generator(None, 2)


def move(ctx, segs, ind, n_env, n_src):
    from var_amd._lib import MoveSeg
    table = (MoveSeg * max(len(segs), 1))(*[MoveSeg(*s) for s in segs])
    return ctx.lib.var_rollout_move(ctx.handle, None, table, len(segs), p(ind), n_env, n_src)


@pytest.mark.parametrize("row_bytes", [1, 4, 12, 16, 27648])
@pytest.mark.parametrize("shift", [0, 1, 4])
def test_move_gathers_rows_at_any_alignment(ctx, row_bytes, shift):
    """T = 3 steps of 5 envs gathered through an index list into (T, 2) rows; shift moves both ends off the 16-byte (1: off
    the 4-byte) grid, so the same row sizes take the 16-byte, the word and the byte path."""
    T, N, nb = 3, 5, 2
    g = torch.Generator().manual_seed(row_bytes + shift)
    src = torch.randint(0, 256, (shift + T * N * row_bytes,), dtype=torch.uint8, generator=g).cuda()
    dst = torch.full((shift + T * nb * row_bytes + 32,), 0xA5, dtype=torch.uint8, device="cuda")
    ind = torch.tensor([4, 1], dtype=torch.int32, device="cuda")
    seg = (src.data_ptr() + shift, dst.data_ptr() + shift, row_bytes, T, N * row_bytes, nb * row_bytes, row_bytes, row_bytes)
    assert move(ctx, [seg], ind, nb, N) == 0
    torch.cuda.synchronize()
    want = src[shift:].view(T, N, row_bytes)[:, [4, 1]].reshape(-1)
    assert torch.equal(dst[shift:shift + want.numel()], want)
    assert (dst[:shift] == 0xA5).all() and (dst[shift + want.numel():] == 0xA5).all()
    dst.fill_(0xA5)
    bad = torch.tensor([5, -1], dtype=torch.int32, device="cuda")            # outside the source: rows left alone, nothing read
    assert move(ctx, [seg], bad, nb, N) == 0
    torch.cuda.synchronize()
    assert (dst == 0xA5).all()


def test_move_refuses_overlap_and_bad_arguments(ctx, var_amd):
    a = torch.arange(64, dtype=torch.float32, device="cuda")
    b = torch.full((64,), SENT, device="cuda")
    ok = (a.data_ptr(), b.data_ptr(), 16, 2, 32, 32, 16, 16)
    cases = {
        "no segments": ([], 2, 2), "17 segments": ([ok] * 17, 2, 2), "row_bytes 0": ([(ok[0], ok[1], 0) + ok[3:]], 2, 2),
        "n_t 0": ([ok[:3] + (0,) + ok[4:]], 2, 2), "negative stride": ([ok[:4] + (-32,) + ok[5:]], 2, 2),
        "src NULL": ([(None,) + ok[1:]], 2, 2), "n_env 0": ([ok], 0, 2), "more envs than the source": ([ok], 3, 2),
        "dst rows overlap": ([ok[:7] + (8,)], 2, 2), "dst steps overlap": ([ok[:5] + (16,) + ok[6:]], 2, 2),
        "dst overlaps src": ([(a.data_ptr(), a.data_ptr() + 16) + ok[2:]], 2, 2),
        "dst overlaps another dst": ([ok, (a.data_ptr(), b.data_ptr() + 32) + ok[2:]], 2, 2),
    }
    for name, (segs, n_env, n_src) in cases.items():
        rcode = move(ctx, segs, None, n_env, n_src)
        assert rcode == -1, name
        with pytest.raises(var_amd.VarHipError):
            ctx.check(rcode, "var_rollout_move")
    torch.cuda.synchronize()
    assert (b == SENT).all() and torch.equal(a, torch.arange(64, dtype=torch.float32, device="cuda"))
    assert move(ctx, [ok], None, 2, 2) == 0
    torch.cuda.synchronize()
    assert torch.equal(b[:16], a[:16]) and (b[16:] == SENT).all()


# ---- minibatches ------------------------------------------------------------------------------------------------------------
def fixture_storage(var_amd, gold):
    T, N = gold["in.reward"].shape[:2]
    cfg = types.SimpleNamespace(RLObsIgnore=['debug'])
    ro = var_amd.RolloutStorage(T, N, {'image': (2, 3, 3), 'pose': (2,), 'debug': (1,)}, Discrete(4), gold["in.hxs"].shape[2], cfg)
    for t in range(T):
        f = lambda k: dev(gold["in." + k][t])                    # noqa: E731
        ro.insert({'image': f("image"), 'pose': f("pose")}, f("hxs"), f("actions"), f("logp"), f("value"), f("reward"), f("masks"),
                  f("bad_masks"))
    return ro


def restated_minibatches(ro, adv, perm, mb):
    stores = {"obs." + k: host(v) for k, v in ro.obs.items()}
    stores.update(actions=host(ro.actions), value_preds=host(ro.value_preds), returns=host(ro.returns), masks=host(ro.masks),
                  action_log_probs=host(ro.action_log_probs), advantages=host(adv))
    return rc.minibatches(stores, host(ro.recurrent_hidden_states), perm, mb)


def sample_dict(sample):
    obs, hxs, actions, vp, ret, masks, old, adv = sample
    d = {"obs." + k: v for k, v in obs.items()}
    d.update(recurrent_hidden_states=hxs, actions=actions, value_preds=vp, returns=ret, masks=masks, action_log_probs=old,
             advantages=adv)
    return {k: host(v) for k, v in d.items()}


def test_minibatches_equal_the_reference_fixture(var_amd, gold):
    ro = fixture_storage(var_amd, gold)
    ro.compute_returns(dev(gold["in.next_value"]), True, rc.GAMMA, rc.LAMBDA, True)
    adv = dev(gold["adv"])                                       # the reference's own advantages: contents compare bit for bit
    torch.manual_seed(GEN_SEED)
    got = [sample_dict(s) for s in ro.recurrent_generator(adv, 2)]
    assert len(got) == 3 and [len(g["actions"]) for g in got] == [14, 14, 7]
    for i in range(int(gold["mb_count"])):                       # the two the reference yields before its IndexError
        for k, v in got[i].items():
            assert v.dtype == gold[f"mb{i}.{k}"].dtype and np.array_equal(v, gold[f"mb{i}.{k}"]), (i, k)
    want = restated_minibatches(ro, adv, gold["perm"], 2)
    for g, w in zip(got, want):
        for k in w:
            assert np.array_equal(g[k], w[k]), k


@pytest.mark.parametrize("T, N, mb", [(1, 1, 1), (7, 5, 2), (4, 8, 8)])
def test_minibatches_equal_the_restatement(var_amd, T, N, mb):
    cfg = types.SimpleNamespace(RLObsIgnore=[])
    ro = var_amd.RolloutStorage(T, N, {'image': (3, 5, 5), 'pose': (3,)}, Box(2), 6, cfg, image_dtype=torch.uint8)
    g = torch.Generator().manual_seed(T * N)
    for x in all_stores(ro).values():
        x.copy_(random_like(x, g))
    ro.returns.copy_(random_like(ro.returns, g))
    adv = torch.randn(T, N, 1, generator=g).cuda()
    torch.manual_seed(GEN_SEED)
    perm = torch.randperm(N).numpy()
    torch.manual_seed(GEN_SEED)
    got = [sample_dict(s) for s in ro.recurrent_generator(adv, mb)]
    want = restated_minibatches(ro, adv, perm, mb)
    assert len(got) == len(want)
    for g_, w in zip(got, want):
        for k in w:
            assert g_[k].shape == w[k].shape and np.array_equal(g_[k], w[k]), k


# ---- the loss head ----------------------------------------------------------------------------------------------------------
class HeadOut:
    def __init__(self, kind, M, n):
        f = lambda *s: torch.full(s, SENT, device="cuda")         # noqa: E731
        self.out, self.g_head, self.g_value, self.logp = f(4), f(M, n), f(M, 1), f(M, 1)
        self.g_logstd = f(n) if kind == 0 else None

    def arrays(self):
        r = {"out": host(self.out), "g_head": host(self.g_head), "g_value": host(self.g_value)}
        if self.g_logstd is not None:
            r["g_logstd"] = host(self.g_logstd)
        return r

    def untouched(self):
        return all(bool((t == SENT).all()) for t in (self.out, self.g_head, self.g_value, self.logp))


def call_head(ctx, kind, d, clipped, o, clip=rc.CLIP, **over):
    M, n = d["head"].shape
    t = {k: (None if v is None else dev(v)) for k, v in d.items()}
    a = dict(head=p(t["head"]), logstd=p(t["logstd"]), value=p(t["value"]), action=p(t["action"]), n=n, M=M, kind=kind, clip=clip,
             out=p(o.out))
    a.update(over)
    return ctx.lib.var_ppo_head(ctx.handle, None, a["kind"], a["head"], a["logstd"], a["value"], a["action"], p(t["old_logp"]),
                                p(t["adv"]), p(t["returns"]), p(t["value_preds"]), a["n"], a["M"], a["clip"], rc.VCOEF, rc.ECOEF,
                                int(clipped), a["out"], p(o.g_head), p(o.g_value), p(o.g_logstd), p(o.logp))


def assert_within(got, ref, dist, what):
    for k, v in ref.items():
        d = float(np.abs(got[k].astype(np.float64).reshape(v.shape) - v).max()) / rc.scale(v)
        print(f"{what} {k}: |gpu - float64| / max |float64| {d:.3e}, torch fp32's own distance {dist[k]:.3e}")
        assert d <= 4 * dist[k], (what, k, d, dist[k])


@pytest.mark.parametrize("clipped", [True, False])
@pytest.mark.parametrize("kind, n", [(0, 1), (0, 2), (0, 4), (1, 1), (1, 8), (1, 16)])
@pytest.mark.parametrize("M", [1, 14, 257, 600])
def test_loss_head_against_float64(ctx, kind, n, M, clipped):
    d = rc.loss_inputs(kind, M, n, 7 * M + n + kind)
    ref = rc.loss_ref(kind, *rc.loss_args(d, clipped))
    o = HeadOut(kind, M, n)
    assert call_head(ctx, kind, d, clipped, o) == 0
    got = o.arrays()
    assert_within(got, ref, rc.loss_distance(kind, M, n, clipped), f"kind {kind} n {n} M {M} clipped {clipped}")
    lp = host(o.logp)[:, 0]
    # (test_gpu_act_step.py's bound for the same arithmetic: about 20 fp32 operations with few-ulp expf / logf)
    assert np.abs(lp - rc.logp64(kind, d["head"], d["logstd"], d["action"])).max() <= 1e-5 * max(1.0, np.abs(lp).max())
    o2 = HeadOut(kind, M, n)                                      # again on the same context: the ticket has rewound
    assert call_head(ctx, kind, d, clipped, o2) == 0
    for k, v in o2.arrays().items():
        assert np.array_equal(bits(v), bits(got[k])), k


@pytest.mark.parametrize("kind, n", [(0, 2), (1, 4)])
def test_loss_head_at_the_exact_kinks(ctx, kind, n):
    """adv = 0 (a tie of the two surrogates), v == vp (l1 == l2, clip gate open), ratio exactly 1 (old_logp = the kernel's own
    log-prob from a first launch): autograd's answers, which the float64 restatement reproduces (test_rollout_host.py)."""
    M = 14
    d = rc.loss_inputs(kind, M, n, 99 + kind)
    o = HeadOut(kind, M, n)
    assert call_head(ctx, kind, d, True, o) == 0
    d["adv"][0] = 0.0
    d["value_preds"][1] = d["value"][1]
    d["old_logp"][2] = host(o.logp)[2]
    ref = rc.loss_ref(kind, *rc.loss_args(d, True))
    o = HeadOut(kind, M, n)
    assert call_head(ctx, kind, d, True, o) == 0
    got = o.arrays()
    assert_within(got, ref, rc.loss_distance(kind, M, n, True), f"kinks kind {kind}")
    lp = host(o.logp)
    assert lp[2, 0] == d["old_logp"][2, 0]                       # ratio = expf(0) = 1: inside the clip range, full gradient
    assert np.abs(got["g_head"][2]).max() > 0
    f = np.float32
    assert got["g_value"][1, 0] == (f(0.5) * f(rc.VCOEF) * (f(1) / f(M))) * (f(2) * (d["value"][1, 0] - d["returns"][1, 0]))
    if kind == 0:
        assert (got["g_head"][0] == 0).all()                     # adv = 0: nothing flows through the ratio
    else:
        zero_adv = dict(d, adv=np.zeros_like(d["adv"]))          # only the entropy term is left in that row
        assert np.allclose(got["g_head"][0], rc.loss_ref(kind, *rc.loss_args(zero_adv, True))["g_head"][0], rtol=1e-4, atol=1e-9)


def test_loss_head_refuses_bad_arguments(ctx, var_amd):
    d = rc.loss_inputs(1, 8, 4, 1)
    g = rc.loss_inputs(0, 8, 2, 1)
    cases = [("kind", 1, d, dict(kind=2)), ("M", 1, d, dict(M=0)), ("n 17", 1, d, dict(n=17)), ("n 0", 1, d, dict(n=0)),
             ("Gaussian n 5", 0, g, dict(n=5)), ("head NULL", 1, d, dict(head=None)), ("logstd NULL", 0, g, dict(logstd=None)),
             ("action NULL", 1, d, dict(action=None)), ("out NULL", 1, d, dict(out=None)), ("clip < 0", 1, d, dict(clip=-0.1)),
             ("clip NaN", 1, d, dict(clip=float("nan")))]
    for name, kind, dd, over in cases:
        o = HeadOut(kind, *dd["head"].shape)
        over = dict(over)
        rcode = call_head(ctx, over.pop("kind", kind), dd, True, o, **over)
        assert rcode == -1, name
        with pytest.raises(var_amd.VarHipError):
            ctx.check(rcode, "var_ppo_head")
        torch.cuda.synchronize()
        assert o.untouched(), name


# ---- ppo_loss and PPO.update ------------------------------------------------------------------------------------------------
class StandIn(torch.nn.Module):
    """A small recurrent-looking actor-critic: two Linear layers per trunk over obs['pose'] and the masked hidden state."""

    def __init__(self, kind, n, hidden=6):
        super().__init__()
        lin = torch.nn.Linear
        self.base = _Base(hidden)
        self.dist = torch.nn.Module()
        if kind == 0:
            self.dist.fc_mean = lin(8, n)
            self.dist.logstd = torch.nn.Module()
            self.dist.logstd._bias = torch.nn.Parameter(torch.tensor([[-0.3], [0.1]][:n]))
        else:
            self.dist.linear = lin(8, n)
    is_recurrent = True


class _Base(torch.nn.Module):
    def __init__(self, hidden):
        super().__init__()
        lin = torch.nn.Linear
        self.critic = torch.nn.Sequential(lin(3 + hidden, 8), torch.nn.Tanh(), lin(8, 1))
        self.actor = torch.nn.Sequential(lin(3 + hidden, 8), torch.nn.Tanh(), lin(8, 8))

    def forward(self, obs, hxs, masks, infer=True):
        T = obs['pose'].shape[0] // hxs.shape[0]
        x = torch.cat([obs['pose'], (hxs.repeat(T, 1) * masks)], dim=1)
        return self.critic(x), self.actor(x), hxs, None


def plain_loss(ac, kind, sample, clipped, dtype):
    """ppo.py:61-87 in plain torch on the module `ac` (any device / dtype)."""
    obs, hxs, actions, vp, ret, masks, old, adv = sample
    c = lambda t: t.to(dtype) if t.is_floating_point() else t    # noqa: E731
    dv = next(ac.parameters()).device
    obs = {k: c(v).to(dv) for k, v in obs.items()}
    hxs, actions, vp, ret, masks, old, adv = (c(t).to(dv) for t in (hxs, actions, vp, ret, masks, old, adv))
    values, feats, _, _ = ac.base(obs, hxs, masks, infer=False)
    if kind == 0:
        mean = ac.dist.fc_mean(feats)
        dist = torch.distributions.Normal(mean, (torch.zeros_like(mean) + ac.dist.logstd._bias.t().view(1, -1)).exp())
        logp = dist.log_prob(actions).sum(-1, keepdim=True)
    else:
        dist = torch.distributions.Categorical(logits=ac.dist.linear(feats))
        logp = dist.log_prob(actions.squeeze(-1)).unsqueeze(-1)
    ent = dist.entropy().mean()
    ratio = torch.exp(logp - old)
    action_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - rc.CLIP, 1.0 + rc.CLIP) * adv).mean()
    if clipped:
        vpc = vp + (values - vp).clamp(-rc.CLIP, rc.CLIP)
        value_loss = 0.5 * torch.max((values - ret).pow(2), (vpc - ret).pow(2)).mean()
    else:
        value_loss = 0.5 * (ret - values).pow(2).mean()
    return value_loss * rc.VCOEF + action_loss - ent * rc.ECOEF, value_loss, action_loss, ent


def filled_rollout(var_amd, kind, n, T, N, seed):
    cfg = types.SimpleNamespace(RLObsIgnore=[])
    ro = var_amd.RolloutStorage(T, N, {'pose': (3,)}, Box(n) if kind == 0 else Discrete(n), 6, cfg)
    g = torch.Generator().manual_seed(seed)
    for t in range(T):
        act = torch.randn(N, n, generator=g) if kind == 0 else torch.randint(0, n, (N, 1), generator=g)
        ro.insert({'pose': torch.randn(N, 3, generator=g).cuda()}, torch.randn(N, 6, generator=g).cuda(), act.cuda(),
                  (torch.randn(N, 1, generator=g) * 0.3 - 1.5).cuda(), torch.randn(N, 1, generator=g).cuda(),
                  torch.randn(N, 1, generator=g).cuda(), (torch.rand(N, 1, generator=g) < 0.8).float().cuda(),
                  torch.ones(N, 1).cuda())
    ro.compute_returns(torch.randn(N, 1, generator=g).cuda(), True, rc.GAMMA, rc.LAMBDA, True)
    return ro


@pytest.mark.parametrize("kind, n", [(0, 2), (1, 4)])
def test_ppo_loss_backward_gives_the_plain_torch_parameter_gradients(var_amd, kind, n):
    """Bound per parameter: four times the distance of plain torch fp32 (on the GPU) from plain torch float64 (CPU)."""
    import copy
    torch.manual_seed(3)
    ac = StandIn(kind, n).cuda()
    ro = filled_rollout(var_amd, kind, n, 5, 4, 17)
    torch.manual_seed(GEN_SEED)
    sample = next(iter(ro.recurrent_generator(ro.advantages(), 2)))
    agent = var_amd.PPO(ac, rc.CLIP, 1, 2, rc.VCOEF, rc.ECOEF, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    outs = agent.loss(sample)
    assert outs[0].requires_grad and not any(o.requires_grad for o in outs[1:])
    outs[0].backward()
    mine = {k: host(v.grad) for k, v in ac.named_parameters()}
    ac32, ac64 = copy.deepcopy(ac), copy.deepcopy(ac).cpu().double()

    def grads(m, smp, dt):
        m.zero_grad()
        ref = plain_loss(m, kind, smp, True, dt)
        ref[0].backward()
        return {k: v.grad.detach().cpu().numpy().astype(np.float64) for k, v in m.named_parameters()}, [float(r.detach()) for r in ref]

    g64, ref64 = grads(ac64, sample, torch.float64)
    for a, b in zip(outs, ref64):                                # fp32 means over 10 rows: 1e-5 is two orders above their rounding
        assert abs(float(a) - b) <= 1e-5 * max(1.0, abs(b))
    dist = {}
    for seed in range(3):                                        # plain fp32's own distance: the largest over six minibatches
        torch.manual_seed(GEN_SEED + seed)
        for smp in ro.recurrent_generator(ro.advantages(), 2):
            a32, b64 = grads(ac32, smp, torch.float32)[0], grads(ac64, smp, torch.float64)[0]
            for k in b64:
                dist[k] = max(dist.get(k, 0.0), float(np.abs(a32[k] - b64[k]).max()))
    for k, g in g64.items():
        d = float(np.abs(mine[k] - g).max())
        print(f"{k}: |ppo_loss - float64| {d:.3e}, plain fp32's own distance {dist[k]:.3e}")
        assert d <= 4 * dist[k], k


@pytest.mark.parametrize("kind, n", [(0, 2), (1, 4)])
def test_update_runs_the_restated_minibatch_sequence(var_amd, kind, n):
    torch.manual_seed(4)
    ac = StandIn(kind, n).cuda()
    T = N = 4
    ro = filled_rollout(var_amd, kind, n, T, N, 23)
    agent = var_amd.PPO(ac, rc.CLIP, 2, 2, rc.VCOEF, rc.ECOEF, lr=1e-3, eps=1e-5, max_grad_norm=0.5)
    seen, gen = [], ro.recurrent_generator

    def recording(advantages, num_mini_batch):
        for s in gen(advantages, num_mini_batch):
            seen.append(sample_dict(s))
            yield s
    ro.recurrent_generator = recording
    before = [v.detach().clone() for v in ac.parameters()]
    torch.manual_seed(GEN_SEED)
    means = agent.update(ro)
    assert len(means) == 3 and all(np.isfinite(m) for m in means)
    assert any(not torch.equal(a, b) for a, b in zip(before, ac.parameters()))
    torch.manual_seed(GEN_SEED)
    want = []
    for _ in range(2):
        want += restated_minibatches(ro, ro.advantages(), torch.randperm(N).numpy(), 2)
    assert len(seen) == 4
    for g_, w in zip(seen, want):
        for k in w:
            assert np.array_equal(g_[k], w[k]), k
    ro.after_update()
    torch.cuda.synchronize()
    assert torch.equal(ro.masks[0], ro.masks[-1]) and torch.equal(ro.obs['pose'][0], ro.obs['pose'][-1])


def test_insert_takes_the_captured_steps_buffers(var_amd):
    """Two steps of IthorNetPolicy.capture(2) go into the storage straight from ActStep's static buffers."""
    cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, RLObsIgnore=[])
    kw = {'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 1024, 'actionHiddenSize': 128}
    torch.manual_seed(11)
    pol = var_amd.IthorNetPolicy(None, Discrete(8), config=cfg, base='ai2thor_VAR', base_kwargs=kw).to("cuda")
    st = pol.capture(2, seed=3)
    shapes = {k: tuple(v.shape[1:]) for k, v in st.obs.items()}
    ro = var_amd.RolloutStorage(2, 2, shapes, Discrete(8), 1024, cfg, image_dtype=torch.uint8)
    g = torch.Generator().manual_seed(2)
    kept = []
    for t in range(2):
        for k, buf in st.obs.items():
            buf.copy_(random_like(buf, g) if buf.dtype == torch.uint8 else torch.nn.functional.normalize(torch.randn(buf.shape, generator=g), dim=1).cuda())
        st.masks.fill_(1.0)
        value, action, logp, hxs = st(st.obs, st.masks)
        reward = torch.randn(2, generator=g).cuda()              # (N,): what IntrinsicReward.step returns
        ro.insert(st.obs, hxs, action, logp, value, reward, st.masks, st.masks)
        kept.append(dict(obs={k: v.clone() for k, v in st.obs.items()}, hxs=hxs.clone(), action=action.clone(), logp=logp.clone(),
                         value=value.clone(), reward=reward.clone()))
    torch.cuda.synchronize()
    for t, kp in enumerate(kept):
        for k in st.obs:
            assert torch.equal(ro.obs[k][t + 1], kp["obs"][k]), k
        assert torch.equal(ro.recurrent_hidden_states[t + 1], kp["hxs"]) and torch.equal(ro.actions[t], kp["action"])
        assert torch.equal(ro.action_log_probs[t], kp["logp"]) and torch.equal(ro.value_preds[t], kp["value"])
        assert torch.equal(ro.rewards[t, :, 0], kp["reward"])
    assert not torch.equal(kept[0]["action"], kept[1]["action"]) or not torch.equal(kept[0]["value"], kept[1]["value"])

"""GPU checks of the Policy.act distribution tail (var_policy_dist, csrc/policy_dist.hip) through the C ABI and of the captured
step (ArmNetPolicy.capture / IthorNetPolicy.capture -> ActStep) against the float64 checker of tests/policy_dist_cpu.py and
against act() itself.

Bounds.  Gaussian action with the caller's noise: 1e-6 -- means ~N(0,1), logstd in [-1, 0] (std <= 1, expf within an ulp:
6e-8 |z|), |z| < 4.5, |action| < 8 (half an ulp of the product and of the sum, 2.4e-7 each): below 8e-7.  Log-probabilities:
|d| <= 1e-5 max(1, |ref|), about 20 fp32 operations with few-ulp expf / logf.  Built-in Gaussian noise: 1e-5 against the float64
Box-Muller of the same uniforms (|z| <= 5.9; the fp32 error of 2 pi u is about 4e-7); an action drawn from it is held to the
checker fed the noise the kernel reports (noise_out / ActStep.noise), which is itself held to the restatement -- the two bounds
in a row are what "follows from the restatement's noise" can mean when z carries 1e-5.  Categorical uniforms are bit-equal.
Categorical actions equal the checker's except where u lies within 1e-5 of a float64 CDF boundary (an fp32 CDF of at most 16
terms is within 1e-6 of it); at most 1 % of the rows may be set aside that way."""
import ctypes
import types

import numpy as np
import pytest
import torch

from tests import policy_dist_cpu as pd

pytestmark = pytest.mark.gpu

ARM_CFG = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, robotStateDim=2)
ARM_KW = {'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 512, 'actionHiddenSize': 128}
ITH_CFG = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3)
ITH_KW = {'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 1024, 'actionHiddenSize': 128}
K0, K1 = 0x9E3779B9, 0x00C0FFEE
SENTINEL = -77.0


class Box:
    shape = (2,)


class Discrete:
    n = 8


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
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def rng_words(k0, k1, step):
    return dev(np.array([k0, k1, step & 0xffffffff, step >> 32], dtype=np.uint32).view(np.int32))


def read_rng(t):
    w = host(t).view(np.uint32)
    return int(w[0]), int(w[1]), (int(w[3]) << 32) | int(w[2])


class Outs:
    """Sentinel-filled outputs of one call."""

    def __init__(self, kind, n, B):
        self.action = (torch.full((B, n), SENTINEL, device="cuda") if kind == 0
                       else torch.full((B, 1), -77, dtype=torch.int64, device="cuda"))
        self.logp = torch.full((B, 1), SENTINEL, device="cuda")
        self.noise = torch.full((B, n) if kind == 0 else (B,), SENTINEL, device="cuda")

    def untouched(self):
        return bool((self.action == -77).all() and (self.logp == SENTINEL).all() and (self.noise == SENTINEL).all())


def call(ctx, kind, head, logstd, n, B, det, noise_in, rng, o, hsrc=None, hdst=None, hidden=0, **over):
    a = dict(head=p(head), logstd=p(logstd), noise_in=p(noise_in), rng=p(rng), noise_out=p(o.noise), action=p(o.action),
             logp=p(o.logp), hsrc=p(hsrc), hdst=p(hdst))
    a.update(over)
    return ctx.lib.var_policy_dist(ctx.handle, None, kind, a['head'], a['logstd'], n, B, int(det), a['noise_in'], a['rng'],
                                   a['noise_out'], a['action'], a['logp'], a['hsrc'], a['hdst'], hidden)


def assert_logp(got, ref):
    d, bound = np.abs(got.astype(np.float64) - ref), 1e-5 * np.maximum(1.0, np.abs(ref))
    assert (d <= bound).all(), (d.max(), ref[np.argmax(d - bound)])


def assert_categorical(logits, u, action, logp):
    """Actions equal the checker's away from the CDF boundaries (at most 1 % of the rows are); logp is that of the GPU's action."""
    B = logits.shape[0]
    ref_a, _ = pd.dist(1, logits, None, u, False)
    skip = pd.near_boundary(logits, u)
    assert skip.sum() <= B // 100, skip.sum()
    assert action.dtype == np.int64 and action.shape == (B, 1)
    assert (action >= 0).all() and (action <= logits.shape[1] - 1).all()
    assert np.array_equal(action[~skip], ref_a[~skip])
    l = logits.astype(np.float64)
    mx = l.max(axis=1, keepdims=True)
    logsm = l - mx - np.log(np.exp(l - mx).sum(axis=1, keepdims=True))
    assert_logp(logp, np.take_along_axis(logsm, action, axis=1))


def gaussian_inputs(n, B, seed):
    r = np.random.default_rng(seed)
    return (r.normal(size=(B, n)).astype(np.float32), r.uniform(-1.0, 0.0, size=n).astype(np.float32),
            r.normal(size=(B, n)).astype(np.float32))


def categorical_inputs(n, B, seed):
    r = np.random.default_rng(seed)
    logits = r.normal(scale=3.0, size=(B, n)).astype(np.float32)
    if n > 1:
        logits[0, n // 2] = logits[0, n - 1] = logits[0].max() + 1.0          # a tie at the maximum: index n // 2 is the mode
    u = r.uniform(size=B).astype(np.float32)
    u[B - 1] = np.float32(1.0 - 2.0 ** -25)                                    # the largest generator value: 1.0f in fp32
    return logits, u


# ---- the kernel through the C ABI, caller's noise ---------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 8, 65])
@pytest.mark.parametrize("n", [1, 2, 4])
def test_gaussian_with_callers_noise(ctx, n, B):
    mean, logstd, z = gaussian_inputs(n, B, 10 * n + B)
    rng = rng_words(K0, K1, 41)
    o = Outs(0, n, B)
    assert call(ctx, 0, dev(mean), dev(logstd), n, B, 0, dev(z), rng, o) == 0
    ref_a, ref_lp = pd.dist(0, mean, logstd, z, False)
    a, lp, used = host(o.action), host(o.logp), host(o.noise)
    print("max |action - ref|", np.abs(a - ref_a).max(), "max |logp - ref|", np.abs(lp - ref_lp).max())
    assert np.abs(a - ref_a).max() <= 1e-6
    assert_logp(lp, ref_lp)
    assert np.array_equal(used, z)                               # noise_out = the noise actually used
    assert read_rng(rng) == (K0, K1, 41)                         # the caller's noise leaves the generator alone
    o = Outs(0, n, B)
    assert call(ctx, 0, dev(mean), dev(logstd), n, B, 1, None, rng, o) == 0
    ref_a, ref_lp = pd.dist(0, mean, logstd, None, True)
    assert np.array_equal(host(o.action), mean)                  # bit-equal to the mean
    assert_logp(host(o.logp), ref_lp)
    assert read_rng(rng) == (K0, K1, 41) and (o.noise == SENTINEL).all()


@pytest.mark.parametrize("B", [1, 8, 65])
@pytest.mark.parametrize("n", [1, 8, 16])
def test_categorical_with_callers_noise(ctx, n, B):
    logits, u = categorical_inputs(n, B, 100 * n + B)
    rng = rng_words(K0, K1, 41)
    o = Outs(1, n, B)
    assert call(ctx, 1, dev(logits), None, n, B, 0, dev(u), rng, o) == 0
    a = host(o.action)
    assert_categorical(logits, u, a, host(o.logp))
    assert a[B - 1, 0] == n - 1                                  # u = 1.0f: every boundary below it, never past n - 1
    assert np.array_equal(host(o.noise), u) and read_rng(rng) == (K0, K1, 41)
    o = Outs(1, n, B)
    assert call(ctx, 1, dev(logits), None, n, B, 1, None, rng, o) == 0
    ref_a, ref_lp = pd.dist(1, logits, None, None, True)
    a = host(o.action)
    assert np.array_equal(a, ref_a) and a[0, 0] == (n // 2 if n > 1 else 0)    # the FIRST index of the largest logit
    assert_logp(host(o.logp), ref_lp)
    assert read_rng(rng) == (K0, K1, 41) and (o.noise == SENTINEL).all()


def test_categorical_4096_rows_of_8_actions(ctx):
    logits, u = categorical_inputs(8, 4096, 5)
    o = Outs(1, 8, 4096)
    assert call(ctx, 1, dev(logits), None, 8, 4096, 0, dev(u), None, o) == 0
    assert_categorical(logits, u, host(o.action), host(o.logp))


# ---- the built-in generator -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [8, 300])
@pytest.mark.parametrize("kind", [0, 1])
def test_builtin_generator_three_launches(ctx, kind, B):
    n, s = (4, 1000) if kind == 0 else (8, 2000)
    r = np.random.default_rng(B + kind)
    head = r.normal(scale=1.0 if kind == 0 else 3.0, size=(B, n)).astype(np.float32)
    logstd = r.uniform(-1.0, 0.0, size=n).astype(np.float32) if kind == 0 else None
    rng = rng_words(K0, K1, s)
    for i in range(3):
        o = Outs(kind, n, B)
        assert call(ctx, kind, dev(head), None if logstd is None else dev(logstd), n, B, 0, None, rng, o) == 0
        used, a, lp = host(o.noise), host(o.action), host(o.logp)
        if kind == 0:
            z = pd.gaussian_noise(K0, K1, s + i, B, n)
            print("max |z - ref|", np.abs(used - z).max())
            assert np.abs(used - z).max() <= 1e-5
            ref_a, ref_lp = pd.dist(0, head, logstd, used, False)
            assert np.abs(a - ref_a).max() <= 1e-6
            assert_logp(lp, ref_lp)
        else:
            u = pd.categorical_noise(K0, K1, s + i, B)
            assert used.dtype == u.dtype and np.array_equal(used.view(np.uint32), u.view(np.uint32))
            assert_categorical(head, used, a, lp)
    assert read_rng(rng) == (K0, K1, s + 3)


@pytest.mark.parametrize("B", [8, 300])
def test_step_low_word_wraps_into_the_high_word(ctx, B):
    logits = np.zeros((B, 8), dtype=np.float32)
    s = (5 << 32) | 0xffffffff
    rng = rng_words(K0, K1, s)
    for i in range(2):
        o = Outs(1, 8, B)
        assert call(ctx, 1, dev(logits), None, 8, B, 0, None, rng, o) == 0
        u = pd.categorical_noise(K0, K1, s + i, B)
        assert np.array_equal(host(o.noise).view(np.uint32), u.view(np.uint32))
    assert read_rng(rng) == (K0, K1, 6 << 32 | 1)


# ---- the distributions themselves -------------------------------------------------------------------------------------------
def test_categorical_counts_fit_softmax(ctx):
    from scipy import stats
    row = np.array([0.3, -0.8, 1.1, 0.0, -1.5, 0.7, -0.2, 0.5], dtype=np.float32)
    B = 4096
    o = Outs(1, 8, B)
    assert call(ctx, 1, dev(np.tile(row, (B, 1))), None, 8, B, 0, None, rng_words(K0, K1, 0), o) == 0
    counts = np.bincount(host(o.action)[:, 0], minlength=8)
    expect = B * pd.softmax_cdf(row[None].astype(np.float64))[0][0]
    chi2 = float(((counts - expect) ** 2 / expect).sum())
    print("chi-square", chi2, "counts", counts)
    assert chi2 < stats.chi2.ppf(1 - 1e-6, 7)                    # 40.52


def test_gaussian_noise_is_normal(ctx):
    from scipy import stats
    B, n = 4096, 2
    o = Outs(0, n, B)
    assert call(ctx, 0, dev(np.zeros((B, n), np.float32)), dev(np.zeros(n, np.float32)), n, B, 0, None, rng_words(K0, K1, 0), o) == 0
    z = host(o.noise)
    assert np.array_equal(host(o.action), z)                     # mean 0, std 1: the action is the noise
    pv = stats.kstest(z.reshape(-1).astype(np.float64), "norm").pvalue
    print("KS p-value", pv)
    assert pv > 1e-6


# ---- the carry ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B, hidden, shift", [(8, 1024, 0), (3, 5, 0), (9, 512, 1), (300, 1024, 0)])
def test_carry_copies_the_state_and_nothing_else(ctx, B, hidden, shift):
    """16-byte pieces when both ends are aligned, single floats otherwise (shift: start one float into the allocation) and for
    the tail; 300 x 1024 floats take more workgroups than the rows do."""
    src = torch.randn(B * hidden + shift, device="cuda")
    dst = torch.full((B * hidden + shift + 8,), SENTINEL, device="cuda")
    logits = torch.zeros(B, 8, device="cuda")
    o = Outs(1, 8, B)
    rng = rng_words(K0, K1, 7)
    assert call(ctx, 1, logits, None, 8, B, 0, None, rng, o, hsrc=src[shift:], hdst=dst[shift:], hidden=hidden) == 0
    torch.cuda.synchronize()
    assert torch.equal(dst[shift:shift + B * hidden], src[shift:]) and (dst[:shift] == SENTINEL).all()
    assert (dst[shift + B * hidden:] == SENTINEL).all()
    assert np.array_equal(host(o.noise).view(np.uint32), pd.categorical_noise(K0, K1, 7, B).view(np.uint32))
    assert read_rng(rng) == (K0, K1, 8)


# ---- error paths ------------------------------------------------------------------------------------------------------------
def test_error_paths_launch_nothing(ctx, var_amd):
    B, hidden = 8, 16
    mean, logstd, z = (dev(a) for a in gaussian_inputs(2, B, 3))
    logits = dev(categorical_inputs(8, B, 3)[0])
    hsrc = torch.randn(B * hidden, device="cuda")
    hdst = torch.full((B * hidden,), SENTINEL, device="cuda")
    cases = [
        ("B < 1", dict(kind=0, n=2, B=0)), ("n < 1", dict(kind=0, n=0)), ("Gaussian n > 4", dict(kind=0, n=5)),
        ("Categorical n > 16", dict(kind=1, n=17)), ("Categorical n < 1", dict(kind=1, n=0)), ("kind", dict(kind=2, n=2)),
        ("head NULL", dict(kind=0, n=2, head=None)), ("logstd NULL", dict(kind=0, n=2, logstd=None)),
        ("action NULL", dict(kind=1, n=8, action=None)), ("logp NULL", dict(kind=1, n=8, logp=None)),
        ("no noise source", dict(kind=1, n=8, rng=None)), ("hxs_dst NULL", dict(kind=1, n=8, hsrc=hsrc, hidden=hidden)),
        ("hxs_dst == hxs_src", dict(kind=1, n=8, hsrc=hsrc, hdst=hsrc, hidden=hidden)),
        ("hidden < 1", dict(kind=1, n=8, hsrc=hsrc, hdst=hdst, hidden=0)),
    ]
    for name, kw in cases:
        kw = dict(kw)                                            # what is left after the pops replaces call()'s own pointer
        kind, n, b, hid = kw.pop("kind"), kw.pop("n"), kw.pop("B", B), kw.pop("hidden", 0)
        o = Outs(kind if kind in (0, 1) else 0, max(n, 1), B)
        rng = rng_words(K0, K1, 9)
        rc = call(ctx, kind, kw.pop("head", mean if kind != 1 else logits), kw.pop("logstd", logstd if kind != 1 else None), n, b,
                  0, None, kw.pop("rng", rng), o, hsrc=kw.pop("hsrc", None), hdst=kw.pop("hdst", None), hidden=hid, **kw)
        assert rc == -1, name                                    # VAR_ERR_ARG
        with pytest.raises(var_amd.VarHipError):
            ctx.check(rc, "var_policy_dist")
        torch.cuda.synchronize()
        assert o.untouched() and (hdst == SENTINEL).all() and read_rng(rng) == (K0, K1, 9), name
    o = Outs(1, 8, B)                                            # and the same arguments, complete, are accepted
    assert call(ctx, 1, logits, None, 8, B, 0, None, rng_words(K0, K1, 9), o, hsrc=hsrc, hdst=hdst, hidden=hidden) == 0
    torch.cuda.synchronize()
    assert torch.equal(hdst, hsrc) and not o.untouched()


# ---- the captured step ------------------------------------------------------------------------------------------------------
def make_policy(var_amd, which, seed=11):
    torch.manual_seed(seed)
    if which == "arm":
        m = var_amd.ArmNetPolicy(None, Box(), config=ARM_CFG, base='arm_VAR', base_kwargs=ARM_KW)
        with torch.no_grad():
            m.dist.logstd._bias.copy_(torch.tensor([[-0.4], [0.2]]))
    else:
        m = var_amd.IthorNetPolicy(None, Discrete(), config=ITH_CFG, base='ai2thor_VAR', base_kwargs=ITH_KW)
        with torch.no_grad():
            m.dist.linear.weight.mul_(100.0)                     # (gain 0.01 leaves the 8 actions all but uniform)
    return m.to("cuda")


@pytest.fixture(scope="module")
def policies(var_amd):
    return {which: make_policy(var_amd, which) for which in ("arm", "ithor")}


def batch(which, B, seed):
    """obs dict and masks on the GPU, seeded as tools/ithor_policy_latency.py draws them."""
    g = torch.Generator().manual_seed(seed)
    obs = {'image': torch.randint(0, 256, (B, 3, 96, 96), dtype=torch.uint8, generator=g).cuda()}
    if which == "ithor":
        obs['occupancy'] = ((torch.rand(B, 1, 9, 9, generator=g) < 0.3).to(torch.uint8) * 255).cuda()
    else:
        obs['robot_pose'] = torch.randn(B, 2, generator=g).cuda()
    obs['image_feat'] = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1).cuda()
    obs['goal_sound_feat'] = torch.nn.functional.normalize(torch.randn(B, 3, generator=g), dim=1).cuda()
    return obs, torch.ones(B, 1, device="cuda")


def assert_step_follows_checker(which, m, st, t, seed):
    """The step's action and logp from its head, the restatement's noise at its rng_step, and the checker."""
    B = st.batch
    assert st.rng_step == t
    head, noise, a, lp = host(st.head), host(st.noise), host(st.action), host(st.action_log_probs)
    if which == "arm":
        z = pd.gaussian_noise(seed & 0xffffffff, seed >> 32, t, B, 2)
        assert np.abs(noise - z).max() <= 1e-5
        ref_a, ref_lp = pd.dist(0, head, host(m.dist.logstd._bias).reshape(-1), noise, False)
        assert np.abs(a - ref_a).max() <= 1e-6
        assert_logp(lp, ref_lp)
    else:
        u = pd.categorical_noise(seed & 0xffffffff, seed >> 32, t, B)
        assert np.array_equal(noise.view(np.uint32), u.view(np.uint32))
        assert_categorical(head, u, a, lp)


@pytest.mark.parametrize("B", [1, 8, 9])
@pytest.mark.parametrize("which", ["arm", "ithor"])
def test_deterministic_steps_equal_act(policies, which, B):
    """8 rows is the last size of the one-launch MLP chain, 9 the first on the per-layer path."""
    m = policies[which]
    st = m.capture(B, deterministic=True)
    hx = torch.randn(B, m.recurrent_hidden_state_size, device="cuda") * 0.3
    st.reset(hx)
    for t in range(3):
        obs, masks = batch(which, B, 50 + t)
        if t == 1:
            masks[0, 0] = 0.0                                    # an episode ends: that row restarts from a zero state
        v, a, lp, hx = m.act(obs, hx, masks, deterministic=True)
        sv, sa, slp, sh = st(obs, masks)
        torch.cuda.synchronize()
        assert torch.equal(sv, v) and torch.equal(sh, hx) and torch.equal(sa, a) and sa.dtype == a.dtype and sa.shape == a.shape
        assert slp.shape == lp.shape and float((slp - lp).abs().max()) <= 1e-5
        assert sa is st.action and sv is st.value
    assert st.rng_step == -1                                     # nothing was drawn
    st.reset()
    assert not bool(st._hxs.any())


@pytest.mark.parametrize("B", [1, 8, 9])
@pytest.mark.parametrize("which", ["arm", "ithor"])
def test_sampled_steps_follow_the_seeded_generator(policies, which, B):
    m = policies[which]
    runs = {}
    for name, seed in (("a", 7), ("b", 7), ("c", (3 << 32) | 8)):
        st = m.capture(B, seed=seed)
        acts = []
        for t in range(4):
            obs, masks = batch(which, B, 60 + t)
            _, a, _, _ = st(obs, masks)
            assert_step_follows_checker(which, m, st, t, seed)
            acts.append(a.clone())
        runs[name] = torch.stack(acts)
    assert torch.equal(runs["a"], runs["b"])
    assert not torch.equal(runs["a"], runs["c"])


@pytest.mark.parametrize("which", ["arm", "ithor"])
def test_step_sees_in_place_updates_and_refuses_a_moved_arena(var_amd, which):
    m = make_policy(var_amd, which, seed=12)
    st = m.capture(8, seed=1)
    obs, masks = batch(which, 8, 70)
    st(obs, masks)
    head0 = st.head.clone()
    with torch.no_grad():
        m.base.actor[0].weight.data.add_(0.05)
    st.reset()
    st(obs, masks)
    torch.cuda.synchronize()
    assert not torch.equal(st.head, head0)
    fresh = m._base_forward(obs, torch.zeros(8, m.recurrent_hidden_state_size, device="cuda"), masks)
    assert torch.equal(st.head, fresh[2]) and torch.equal(st.value, fresh[0])
    m.to("cuda")                                                 # re-flattens the arena: the graph's addresses are stale
    with pytest.raises(var_amd.VarHipError):
        st(obs, masks)
    st2 = m.capture(8, seed=1)
    st2(obs, masks)
    torch.cuda.synchronize()
    assert torch.equal(st2.head, fresh[2])


@pytest.mark.parametrize("which", ["arm", "ithor"])
def test_200_replays_stay_clean(policies, which):
    m = policies[which]
    m.clear_chain_status()
    st = m.capture(8, seed=7)
    obs, masks = batch(which, 8, 80)
    for t in range(200):
        out = st(obs, masks)
    assert m.chain_status() == 0
    assert all(bool(torch.isfinite(x.float()).all()) for x in out)
    assert_step_follows_checker(which, m, st, 199, 7)


def test_argument_checks(var_amd, policies):
    m = policies["ithor"]
    st = m.capture(8)
    obs, masks = batch("ithor", 8, 90)
    with pytest.raises(var_amd.VarHipError):
        st({k: v.cpu() for k, v in obs.items()}, masks)
    with pytest.raises(var_amd.VarHipError):
        st(obs, masks.cpu())
    with pytest.raises(var_amd.VarHipError):
        st({k: v[:4] for k, v in obs.items()}, masks[:4])
    with pytest.raises(var_amd.VarHipError):
        st({k: v for k, v in obs.items() if k != 'occupancy'}, masks)
    with pytest.raises(var_amd.VarHipError):
        st({**obs, 'image': obs['image'].float() / 255.}, masks)             # captured for uint8 images
    with pytest.raises(var_amd.VarHipError):
        st.reset(torch.zeros(8, 512, device="cuda"))
    with pytest.raises(var_amd.VarHipError):
        m.capture(0)
    f = m.capture(8, deterministic=True, image_dtype=torch.float32)
    fobs = {**obs, 'image': obs['image'].float() / 255., 'occupancy': obs['occupancy'].float() / 255.}
    v, a, lp, h = m.act(fobs, torch.zeros(8, 1024, device="cuda"), masks, deterministic=True)
    fv, fa, _, fh = f(fobs, masks)
    torch.cuda.synchronize()
    assert torch.equal(fv, v) and torch.equal(fa, a) and torch.equal(fh, h)
    with pytest.raises(NotImplementedError):
        m.evaluate_actions(None, None, None, None)


def test_ithor_step_chains_with_the_reward_step(var_amd, policies):
    """image_feat / goal_sound_feat straight from IntrinsicReward.step's device tensors: the same as passing clones."""
    m = policies["ithor"]
    torch.manual_seed(5)
    enc = var_amd.IthorVARPretextNet(types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 600, 40), representationDim=3))
    rew = var_amd.IntrinsicReward(enc.to("cuda").eval()).capture(8)
    obs, masks = batch("ithor", 8, 95)
    g = torch.Generator().manual_seed(96)
    goal = (torch.randn(8, 1, 600, 40, generator=g) * 6.0).cuda()
    image_feat, goal_feat, _ = rew.step(obs['image'], goal)
    st = m.capture(8, deterministic=True)
    chained = [t.clone() for t in st({**obs, 'image_feat': image_feat, 'goal_sound_feat': goal_feat}, masks)]
    st.reset()
    cloned = st({**obs, 'image_feat': image_feat.clone(), 'goal_sound_feat': goal_feat.clone()}, masks)
    torch.cuda.synchronize()
    for x, y in zip(chained, cloned):
        assert torch.equal(x, y)
    want = m.act({**obs, 'image_feat': image_feat, 'goal_sound_feat': goal_feat}, torch.zeros(8, 1024, device="cuda"), masks,
                 deterministic=True)
    assert torch.equal(cloned[0], want[0]) and torch.equal(cloned[1], want[1]) and torch.equal(cloned[3], want[3])

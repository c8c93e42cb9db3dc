"""GPU parity of the iTHOR actor-critic forward (var_ithor_policy_forward through IthorNetPolicy.act) against the fixture
the reference's Policy(base='ai2thor_VAR') produced (tests/golden/ithor_policy_b8.npz), against the torch-CPU restatement
(tests/ithor_policy_cpu.py) with identical weights, and across its kernel paths (band convolutions / gather-GEMM, one-launch
MLP chain / one launch per layer)."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests.ithor_policy_cpu import forward as cpu_forward

pytestmark = pytest.mark.gpu

CFG = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3)
KW = {'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 1024, 'actionHiddenSize': 128}


class Discrete:
    def __init__(self, n):
        self.n = n


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available()
    return m


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ithor_policy_b8.npz")))


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def make(var_amd, seed, n=8):
    nt = torch.get_num_threads()
    torch.set_num_threads(4)                       # (the fixture's weights: see test_ithor_policy_host.py)
    try:
        torch.manual_seed(seed)
        m = var_amd.IthorNetPolicy(None, Discrete(n), config=CFG, base='ai2thor_VAR', base_kwargs=KW)
    finally:
        torch.set_num_threads(nt)
    return m.to("cuda")


def obs_of(fx, u8):
    img, occ = cuda(fx['image']), cuda(fx['occupancy'])
    return {'image': img if u8 else (img / 255.).float(), 'occupancy': occ if u8 else (occ / 255.).float(),
            'image_feat': cuda(fx['image_feat']), 'goal_sound_feat': cuda(fx['goal_sound_feat'])}


def cpu_ref(m, obs, hxs, masks):
    f = lambda t: t.detach().cpu()                 # noqa: E731
    img, occ = f(obs['image']), f(obs['occupancy'])
    img = img.float() / 255. if img.dtype == torch.uint8 else img
    occ = occ.float() / 255. if occ.dtype == torch.uint8 else occ
    with torch.no_grad():
        return cpu_forward(m.state_dict(), img, occ, f(obs['image_feat']), f(obs['goal_sound_feat']), f(hxs), f(masks))


def random_batch(n, seed):
    g = torch.Generator().manual_seed(seed)
    obs = {'image': torch.randint(0, 256, (n, 3, 96, 96), dtype=torch.uint8, generator=g).cuda(),
           'occupancy': ((torch.rand(n, 1, 9, 9, generator=g) < 0.3).to(torch.uint8) * 255).cuda(),
           'image_feat': torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1).cuda(),
           'goal_sound_feat': torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1).cuda()}
    hxs = torch.randn(n, 1024, generator=g).cuda() * 0.3
    masks = (torch.rand(n, 1, generator=g) > 0.2).float().cuda()
    return obs, hxs, masks


def close(got, want, atol, msg=""):
    np.testing.assert_allclose(got.detach().cpu().numpy(), want.detach().cpu().numpy() if torch.is_tensor(want) else want,
                               rtol=0, atol=atol, err_msg=msg)


def test_act_vs_reference_fixture(var_amd, fx):
    m = make(var_amd, int(fx["seed"]))
    assert [k for k, _ in m.state_dict().items()] == [str(k) for k in fx["names"]]
    assert m.is_recurrent and m.recurrent_hidden_state_size == 1024
    for u8 in (True, False):
        obs = obs_of(fx, u8)
        v, a, lp, h = m.act(obs, cuda(fx['rnn_hxs']), cuda(fx['masks']), deterministic=True)
        v2, a2, lp2, h2 = m.act(obs, h, torch.ones(8, 1, device="cuda"), deterministic=True)
        assert a.dtype == torch.int64 and a.shape == (8, 1) and lp.shape == (8, 1)
        for got, name in ((v, 'value'), (lp, 'action_log_probs'), (h, 'rnn_hxs_out'), (v2, 'value2'),
                          (lp2, 'action_log_probs2'), (h2, 'rnn_hxs_out2')):
            close(got, fx[name], 1e-4, f"{name} u8={u8}")
        np.testing.assert_array_equal(a.cpu().numpy(), fx['action'])
        np.testing.assert_array_equal(a2.cpu().numpy(), fx['action2'])
        value, feats, logits, _ = m._base_forward(obs, cuda(fx['rnn_hxs']), cuda(fx['masks']))
        close(feats, fx['actor_features'], 1e-4, "actor_features")
        close(logits, fx['logits'], 1e-4, "logits")


def test_sampling_get_value_and_rejections(var_amd, fx):
    m = make(var_amd, int(fx["seed"]))
    obs, hxs, masks = obs_of(fx, True), cuda(fx['rnn_hxs']), cuda(fx['masks'])
    torch.manual_seed(0)
    v, a, lp, h = m.act(obs, hxs, masks)
    assert a.shape == (8, 1) and a.dtype == torch.int64 and ((a >= 0) & (a < 8)).all()
    _, _, logits, _ = m._base_forward(obs, hxs, masks)
    want = torch.distributions.Categorical(logits=logits).log_prob(a.squeeze(-1)).unsqueeze(-1)
    close(lp, want, 1e-6)
    close(m.get_value(obs, hxs, masks), v, 0)
    with pytest.raises(NotImplementedError):
        m.evaluate_actions(None, None, None, None)
    with pytest.raises(var_amd.VarHipError):
        m.act({k: t.cpu() for k, t in obs.items()}, hxs, masks)
    # in-place state update is refused
    from var_amd._lib import Context
    ctx = Context.get(0)
    f = lambda t: ctypes.c_void_p(t.data_ptr())    # noqa: E731
    img, occ = obs['image'].contiguous(), obs['occupancy'].contiguous()
    out = [torch.empty(8, n, device="cuda") for n in (1, 128, 8)]
    hh = hxs.clone()
    rc = ctx.lib.var_ithor_policy_forward(ctx.handle, None, f(m._flat), 8, f(img), 1, img.stride(0), f(occ), 1,
                                          f(obs['image_feat']), f(obs['goal_sound_feat']), f(hh), f(masks), 8,
                                          f(out[0]), f(out[1]), f(out[2]), f(hh))
    assert rc != 0
    with pytest.raises(var_amd.VarHipError):
        ctx.check(rc, "var_ithor_policy_forward")


@pytest.mark.parametrize("B", [1, 5, 8])
def test_chain_equals_the_per_layer_path_and_cpu(var_amd, fx, B):
    """B <= 8 takes the one-launch MLP chain (csrc/chain.h) after the convolutions; larger batches one launch per layer.
    The same rows through both (alone, and as the first rows of a batch of 12), two consecutive steps."""
    m = make(var_amd, 7)
    obs, hxs, masks = random_batch(12, 5)
    small = {k: v[:B].contiguous() for k, v in obs.items()}
    o1 = m._base_forward(small, hxs[:B].contiguous(), masks[:B].contiguous())
    o2 = m._base_forward(obs, hxs, masks)
    for got, want in zip(o1, o2):
        close(got, want[:B], 2e-5)
    for got, want in zip(o1, cpu_ref(m, small, hxs[:B], masks[:B])):
        close(got, want, 2e-5)
    for got, want in zip(o2, cpu_ref(m, obs, hxs, masks)):
        close(got, want, 2e-5)
    # get_value runs the same forward without the logit layer (a NULL head): the value's bits must not depend on it
    close(m.get_value(small, hxs[:B].contiguous(), masks[:B].contiguous()),
          m.act(small, hxs[:B].contiguous(), masks[:B].contiguous(), deterministic=True)[0], 0)
    close(m.get_value(obs, hxs, masks), m.act(obs, hxs, masks, deterministic=True)[0], 0)
    o3 = m._base_forward(small, o1[3], torch.ones(B, 1, device="cuda"))
    o4 = m._base_forward(obs, o2[3], torch.ones(12, 1, device="cuda"))
    for got, want in zip(o3, o4):
        close(got, want[:B], 5e-5)


def test_band_convolutions_equal_the_gather_gemm_path(var_amd, fx):
    """Up to 64 images the image stack runs on the LDS-band kernels of csrc/c3f.h; larger batches on the gather-GEMM + pool
    launches.  The same rows alone (B = 8: band + chain, B = 64: band + per layer) and inside a batch of 70."""
    m = make(var_amd, 9)
    obs, hxs, masks = random_batch(70, 11)
    big = m._base_forward(obs, hxs, masks)
    for got, want in zip(big, cpu_ref(m, obs, hxs, masks)):
        close(got, want, 2e-5)
    for B in (8, 64):
        small = {k: v[:B].contiguous() for k, v in obs.items()}
        o = m._base_forward(small, hxs[:B].contiguous(), masks[:B].contiguous())
        for got, want in zip(o, big):
            close(got, want[:B], 2e-5, f"B={B}")
    # float inputs take the other instantiation of the u8 kernels
    fl = {k: (v[:8].float() / 255. if v.dtype == torch.uint8 else v[:8].contiguous()) for k, v in obs.items()}
    o = m._base_forward(fl, hxs[:8].contiguous(), masks[:8].contiguous())
    for got, want in zip(o, big):
        close(got, want[:8], 2e-5, "f32")


def test_replayed_forward_is_stable_and_sees_new_inputs_and_weights(var_amd, fx):
    """200 replays of one captured forward return the first replay's bits (the chain's hand-over epoch lives on the
    device), follow the static input buffers and the parameters changed in place; the chain status stays clean."""
    m = make(var_amd, int(fx["seed"]))
    obs = {k: v.clone() for k, v in obs_of(fx, True).items()}
    hxs, masks = cuda(fx['rnn_hxs']).clone(), cuda(fx['masks']).clone()
    eager = [t.clone() for t in m._base_forward(obs, hxs, masks)]
    g = var_amd._lib.new_graph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m._base_forward(obs, hxs, masks)
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            outs = m._base_forward(obs, hxs, masks)
    torch.cuda.synchronize()
    g.replay()
    torch.cuda.synchronize()
    first = [t.clone() for t in outs]
    for a, b in zip(first, eager):
        assert torch.equal(a, b)
    for i in range(200):
        g.replay()
        if i % 50 == 49:
            torch.cuda.synchronize()
            for a, b in zip(outs, first):
                assert torch.equal(a, b), f"replay {i}"
    obs['goal_sound_feat'].mul_(-1.0)
    obs['occupancy'].copy_(255 - obs['occupancy'])
    obs['image'].copy_(torch.flip(obs['image'], dims=[3]))
    want = [t.clone() for t in m._base_forward(obs, hxs, masks)]
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, want):
        assert torch.equal(a, b)
    assert not torch.equal(outs[0], first[0])
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.01)
    want = [t.clone() for t in m._base_forward(obs, hxs, masks)]
    g.replay()
    torch.cuda.synchronize()
    for a, b in zip(outs, want):
        assert torch.equal(a, b)
    assert m.chain_status() == 0
    m.clear_chain_status()
    assert m.chain_status() == 0


def test_reference_layout_state_dict_round_trip(var_amd, fx):
    src = make(var_amd, 3)
    dst = make(var_amd, 4)
    sd = {k: v.detach().cpu().clone() for k, v in src.state_dict().items()}
    dst.load_state_dict(sd)
    back = dst.state_dict()
    assert list(back.keys()) == list(sd.keys())
    for k in sd:
        assert torch.equal(back[k].cpu(), sd[k]), k
    obs, hxs, masks = obs_of(fx, True), cuda(fx['rnn_hxs']), cuda(fx['masks'])
    for a, b in zip(src._base_forward(obs, hxs, masks), dst._base_forward(obs, hxs, masks)):
        assert torch.equal(a, b)

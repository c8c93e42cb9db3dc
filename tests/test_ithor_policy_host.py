"""Host-side checks of the iTHOR actor-critic (IthorNetPolicy, base 'ai2thor_VAR'): the seeded construction reproduces
the reference Policy's 64 tensors bit for bit (tests/golden/ithor_policy_b8.npz, made by make_golden_ithor_policy.py),
the torch-CPU restatement (tests/ithor_policy_cpu.py) reproduces the reference's outputs on those weights, the
configuration checks, the Policy() dispatch and the C ABI's parameter count.  No GPU needed."""
import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests.ithor_policy_cpu import forward as cpu_forward

CFG = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3)
KW = {'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 1024, 'actionHiddenSize': 128}


class Discrete:
    def __init__(self, n):
        self.n = n


class Box:
    def __init__(self, n):
        self.shape = (n,)


@pytest.fixture(scope="module")
def fx(golden_dir):
    return dict(np.load(os.path.join(golden_dir, "ithor_policy_b8.npz")))


@pytest.fixture(scope="module")
def seeded(fx):
    import var_amd
    # orthogonal_ goes through a LAPACK QR whose last bits depend on the thread count: the fixture was made with 4 threads
    nt = torch.get_num_threads()
    torch.set_num_threads(4)
    try:
        torch.manual_seed(int(fx["seed"]))
        return var_amd.IthorNetPolicy(None, Discrete(8), config=CFG, base='ai2thor_VAR', base_kwargs=KW)
    finally:
        torch.set_num_threads(nt)


def check_values(v):
    f = v.reshape(-1).astype(np.float64)
    return np.concatenate([[f.sum(), np.abs(f).sum()], f[:8]])


def test_seeded_construction_matches_reference_tensors(fx, seeded):
    sd = seeded.state_dict()
    assert list(sd.keys()) == [str(k) for k in fx["names"]]
    assert len(sd) == 64 and sum(v.numel() for v in sd.values()) == 5475081
    for k, v in sd.items():
        assert tuple(v.shape) == tuple(fx["shape." + k]), k
        np.testing.assert_array_equal(check_values(v.numpy()), fx["check." + k], err_msg=k)
    assert seeded.is_recurrent and seeded.recurrent_hidden_state_size == 1024


def test_cpu_restatement_reproduces_reference_outputs(fx, seeded):
    sd = seeded.state_dict()
    t = lambda k: torch.from_numpy(fx[k])                     # noqa: E731
    img, occ = t('image').float() / 255., t('occupancy').float() / 255.
    with torch.no_grad():
        v, f, lg, h = cpu_forward(sd, img, occ, t('image_feat'), t('goal_sound_feat'), t('rnn_hxs'), t('masks'))
        v2, f2, lg2, h2 = cpu_forward(sd, img, occ, t('image_feat'), t('goal_sound_feat'), h, torch.ones(8, 1))
    dist = torch.distributions.Categorical(logits=lg)
    a = dist.probs.argmax(-1, keepdim=True)
    lp = dist.log_prob(a.squeeze(-1)).unsqueeze(-1)
    dist2 = torch.distributions.Categorical(logits=lg2)
    a2 = dist2.probs.argmax(-1, keepdim=True)
    lp2 = dist2.log_prob(a2.squeeze(-1)).unsqueeze(-1)
    for got, name in ((v, 'value'), (f, 'actor_features'), (lg, 'logits'), (h, 'rnn_hxs_out'), (lp, 'action_log_probs'),
                      (v2, 'value2'), (f2, 'actor_features2'), (h2, 'rnn_hxs_out2'), (lp2, 'action_log_probs2')):
        np.testing.assert_allclose(got.numpy(), fx[name], rtol=0, atol=1e-5, err_msg=name)
    np.testing.assert_array_equal(a.numpy(), fx['action'])
    np.testing.assert_array_equal(a2.numpy(), fx['action2'])


def test_configuration_checks():
    import var_amd
    with pytest.raises(NotImplementedError):
        var_amd.IthorNetPolicy(None, Box(2), config=CFG, base='ai2thor_VAR', base_kwargs=KW)
    with pytest.raises(NotImplementedError):
        var_amd.IthorNetPolicy(None, Discrete(8), config=CFG, base='arm_VAR', base_kwargs=KW)
    bad = [(types.SimpleNamespace(img_dim=(3, 84, 84), representationDim=3), KW, 8),
           (CFG, dict(KW, recurrent=False), 8),
           (CFG, dict(KW, recurrentSize=512), 8),
           (CFG, dict(KW, recurrentInputSize=64), 8),
           (CFG, dict(KW, actionHiddenSize=64), 8),
           (CFG, KW, 17)]
    for cfg, kw, n in bad:
        with pytest.raises(var_amd.VarHipError):
            var_amd.IthorNetPolicy(None, Discrete(n), config=cfg, base='ai2thor_VAR', base_kwargs=kw)
    m = var_amd.IthorNetPolicy(None, Discrete(4), config=CFG, base='ai2thor_VAR', base_kwargs=KW)
    with pytest.raises(NotImplementedError):
        m.evaluate_actions(None, None, None, None)
    # CPU module / CPU inputs: no fallback
    obs = {'image': torch.zeros(2, 3, 96, 96, dtype=torch.uint8), 'occupancy': torch.zeros(2, 1, 9, 9, dtype=torch.uint8),
           'image_feat': torch.zeros(2, 3), 'goal_sound_feat': torch.zeros(2, 3)}
    with pytest.raises(var_amd.VarHipError):
        m.act(obs, torch.zeros(2, 1024), torch.ones(2, 1))


def test_policy_dispatches_both_bases():
    import var_amd
    a = var_amd.Policy(None, Discrete(8), config=CFG, base='ai2thor_VAR', base_kwargs=KW)
    assert isinstance(a, var_amd.IthorNetPolicy) and a.n_actions == 8
    kcfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, robotStateDim=2)
    kkw = {'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 512, 'actionHiddenSize': 128}
    k = var_amd.Policy(None, Box(2), config=kcfg, base='arm_VAR', base_kwargs=kkw)
    assert isinstance(k, var_amd.ArmNetPolicy)
    for base in (None, 'cnn'):
        with pytest.raises(NotImplementedError):
            var_amd.Policy(None, Discrete(8), config=CFG, base=base, base_kwargs=KW)


def test_c_abi_parameter_count():
    import var_amd
    lib = ctypes.CDLL(var_amd.library_path())
    assert lib.var_ithor_policy_param_count(8) == 5475081
    for n in (1, 16):
        m = var_amd.IthorNetPolicy(None, Discrete(n), config=CFG, base='ai2thor_VAR', base_kwargs=KW)
        assert lib.var_ithor_policy_param_count(n) == sum(p.numel() for p in m.parameters())
    assert lib.var_ithor_policy_param_count(0) < 0 and lib.var_ithor_policy_param_count(17) < 0

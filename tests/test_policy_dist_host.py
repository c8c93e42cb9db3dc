"""CPU-side checks of the Policy.act distribution tail: the checker (tests/policy_dist_cpu.py) against published Philox
answers and against torch.distributions in float64, and the binding of var_policy_dist / ActStep (no compute is called)."""
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import policy_dist_cpu as pd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("ctr, key, want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
])
def test_philox_known_answers(ctr, key, want):
    got = pd.philox4x32_10(np.array(ctr, dtype=np.uint64), np.array(key, dtype=np.uint64))
    assert [int(x) for x in got] == list(want)


def test_philox_is_vectorised_over_rows_and_uniform_mapping():
    w = pd.words(0xa4093822, 0x299f31d0, (0x85a308d3 << 32) | 0x243f6a88, np.arange(5))
    for r in range(5):
        one = pd.philox4x32_10(np.array([0x243f6a88, 0x85a308d3, r, 0], dtype=np.uint64),
                               np.array([0xa4093822, 0x299f31d0], dtype=np.uint64))
        assert np.array_equal(w[r], one)
    u = pd.uniform(np.array([0, 0xff, 0x100, 0x7fffffff, 0x80000000, 0xffffffff], dtype=np.uint32))
    assert u.dtype == np.float32
    assert u[0] == u[1] == np.float32(2.0 ** -25) and u[2] == np.float32(1.5 * 2.0 ** -24)
    assert u[3] == np.float32((2 ** 23 - 0.5) * 2.0 ** -24)          # the last exactly representable sum
    assert u[4] == np.float32(0.5) and u[5] == np.float32(1.0)       # 2^23 + 0.5 -> 2^23, 2^24 - 0.5 -> 2^24 (to even)
    z = pd.gaussian_noise(1, 2, 3, 64, 4)
    assert z.shape == (64, 4) and np.isfinite(z).all() and np.abs(z).max() < 5.9


@pytest.mark.parametrize("n", [1, 2, 4])
def test_gaussian_checker_equals_torch(n):
    rng = np.random.default_rng(100 + n)
    mean, logstd, z = rng.normal(size=(33, n)), rng.uniform(-1.0, 0.5, size=n), rng.normal(size=(33, n))
    for det in (False, True):
        a, lp = pd.dist(0, mean, logstd, z, det)
        d = torch.distributions.Normal(torch.from_numpy(mean), torch.from_numpy(np.exp(logstd)).expand(33, n))
        want_a = mean if det else mean + np.exp(logstd) * z
        assert np.abs(a - want_a).max() <= 1e-12
        want = d.log_prob(torch.from_numpy(a)).sum(-1, keepdim=True).numpy()
        assert lp.shape == (33, 1) and np.abs(lp - want).max() <= 1e-12


@pytest.mark.parametrize("n", [1, 5, 16])
def test_categorical_checker_equals_torch(n):
    rng = np.random.default_rng(200 + n)
    logits = rng.normal(scale=3.0, size=(257, n))
    if n > 1:
        logits[3, 1] = logits[3, n - 1] = logits[3].max() + 1.0      # a tie at the maximum: the first index wins
    u = rng.uniform(size=257)
    u[0], u[1] = 1.0, 2.0 ** -25                                     # the generator's extremes
    d = torch.distributions.Categorical(logits=torch.from_numpy(logits))
    a, lp = pd.dist(1, logits, None, u, False)
    assert a.dtype == np.int64 and a.shape == (257, 1) and a.min() >= 0 and a.max() <= n - 1
    assert a[0, 0] == n - 1
    # inverse CDF: the action is the first k whose cumulative probability exceeds u
    cdf = np.cumsum(d.probs.numpy(), axis=1)
    for r in range(257):
        k = int(a[r, 0])
        assert (k == 0 or cdf[r, k - 1] <= u[r]) and (k == n - 1 or u[r] < cdf[r, k])
    assert np.abs(lp - d.log_prob(torch.from_numpy(a[:, 0])).unsqueeze(-1).numpy()).max() <= 1e-12
    am, lpm = pd.dist(1, logits, None, None, True)
    assert np.array_equal(am, d.probs.argmax(dim=-1, keepdim=True).numpy())
    if n > 1:
        assert am[3, 0] == 1
    assert np.abs(lpm - d.log_prob(torch.from_numpy(am[:, 0])).unsqueeze(-1).numpy()).max() <= 1e-12
    assert not pd.near_boundary(logits, np.full(257, -1.0)).any()
    if n > 1:
        assert pd.near_boundary(logits, cdf[:, 0]).all()


def test_var_policy_dist_is_declared_and_bound():
    import ctypes
    import var_amd
    from var_amd._lib import _SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "var_hip.h")).read()
    assert re.search(r"\bint\s+var_policy_dist\s*\(", hdr)
    res, args = _SIGNATURES["var_policy_dist"]
    vp, i = ctypes.c_void_p, ctypes.c_int
    assert res is i
    assert args == [vp, vp, i, vp, vp, i, i, i, vp, vp, vp, vp, vp, vp, vp, i]
    lib = var_amd.load_library()
    assert lib.var_policy_dist.argtypes == args
    # no context: refused before anything touches a device
    assert lib.var_policy_dist(None, None, 1, None, None, 8, 8, 0, None, None, None, None, None, None, None, 0) == -1


def test_act_step_is_exported_and_capture_needs_the_gpu_model():
    import var_amd

    class Box:
        shape = (2,)

    class Discrete:
        n = 8
    assert isinstance(var_amd.ActStep, type)
    arm = var_amd.ArmNetPolicy(None, Box(), config=types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, robotStateDim=2),
                               base='arm_VAR', base_kwargs={'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 512,
                                                            'actionHiddenSize': 128})
    ith = var_amd.IthorNetPolicy(None, Discrete(), config=types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3),
                                 base='ai2thor_VAR', base_kwargs={'recurrent': True, 'recurrentInputSize': 128,
                                                                  'recurrentSize': 1024, 'actionHiddenSize': 128})
    for pol in (arm, ith):                                           # CPU-resident: loud, no fallback
        with pytest.raises(var_amd.VarHipError):
            pol.capture(8)
        with pytest.raises(var_amd.VarHipError):
            pol.capture(8, deterministic=True, seed=7)
        with pytest.raises(NotImplementedError):
            pol.evaluate_actions(None, None, None, None)

"""Host checks of the float64 restatement of var_ppo_head_linear (tests/ppo_head_linear_cpu.py) and of the bounds the GPU test
takes from it: torch's own fp32 evaluation lies inside them on draws the bounds were not made from, and each of four injected
faults -- a dropped bias, W transposed, g_b taken from g_value, one row left out of g_W -- fails exactly its own array."""
import numpy as np
import pytest
import torch

from tests import ppo_head_linear_cpu as hl
from tests import rollout_cpu as rc

CASES = [(0, 2, 37, True), (0, 4, 257, False), (1, 8, 37, True), (1, 16, 257, True), (1, 2, 300, False)]


def failing(kind, n, M, clipped, seed, fault=None):
    d, _ = hl.inputs(kind, M, n, seed)
    err = hl.errors(hl.torch32(kind, d, clipped, fault=fault), hl.ref(kind, d, clipped))
    bound = hl.bounds(kind, M, n, clipped)
    assert set(err) == set(bound) == set(hl.ARRAYS) - (set() if kind == 0 else {"g_logstd"})
    return sorted(k for k in err if not err[k] <= bound[k]), err, bound


def test_restated_gradients_equal_float64_autograd():
    """The closed forms behind the Linear against torch autograd in float64, through the Linear."""
    for kind, n, M, clipped in CASES:
        d, _ = hl.inputs(kind, M, n, 3)
        want = hl.ref(kind, d, clipped)
        f, W, b = (torch.from_numpy(d[k]).double().requires_grad_() for k in ("features", "W", "b"))
        head = torch.nn.functional.linear(f, W, b)
        res = rc.loss_torch(kind, head.detach().numpy(), d["logstd"], d["value"], d["action"], d["old_logp"], d["adv"], d["returns"],
                            d["value_preds"], rc.CLIP, rc.VCOEF, rc.ECOEF, clipped, dtype=torch.float64)
        head.backward(torch.from_numpy(res["g_head"]))
        got = dict(res, head=head.detach().numpy(), g_features=f.grad.numpy(), g_W=W.grad.numpy(), g_b=b.grad.numpy())
        for k, e in hl.errors(got, want).items():
            assert e <= 1e-12, (kind, n, M, k, e)


@pytest.mark.parametrize("kind,n,M,clipped", CASES)
def test_torch_fp32_lies_inside_the_bounds(kind, n, M, clipped):
    for seed in (1, 2, 3):
        bad, err, bound = failing(kind, n, M, clipped, seed)
        assert not bad, (bad, err, bound)


@pytest.mark.parametrize("fault", sorted(hl.FAULTS))
@pytest.mark.parametrize("kind,n,M,clipped", CASES)
def test_an_injected_fault_fails_exactly_its_own_array(kind, n, M, clipped, fault):
    bad, err, bound = failing(kind, n, M, clipped, 1, fault)
    assert bad == [hl.FAULTS[fault]], (fault, bad, err, bound)


def test_few_rows_are_drawn_again():
    for kind, n, M, _ in CASES:
        _, redrawn = hl.inputs(kind, M, n, 5)
        assert redrawn * 10 <= M, (kind, n, M, redrawn)


def test_the_bounds_are_fp32_sized():
    """A bound is a few fp32 roundings of a 128-term dot product or an M-row sum, never a loose one."""
    for kind, n, M, clipped in CASES:
        for k, v in hl.bounds(kind, M, n, clipped).items():
            assert 0 < v < 1e-4, (kind, n, M, k, v)
    assert np.float32(1) + np.float32(2.0 ** -24) == np.float32(1)

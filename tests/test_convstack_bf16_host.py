"""Host checks of the convolution stacks' bf16 mode: the layer-by-layer CPU restatement (tests/convstack_bf16_cpu.py) against
convstack_cpu.evaluate, the non-triviality of every case the GPU file uses, the workspace query of the _ex entries on the library
as it loads without a GPU, and the wrapper's refusal of an unknown precision before it touches a device."""
import numpy as np
import pytest
import torch

from tests import convstack_bf16_cpu as cb
from tests import convstack_cpu as cc


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_the_helper_without_rounding_is_the_float64_evaluation(kind):
    P, d = cc.convstack_params(kind, 5), cc.convstack_data(kind, 2, 5)
    ref = cc.evaluate(kind, P, d, torch.float64)
    got = cb.chain(kind, P, d, torch.float64, rounding=False)
    assert np.allclose(got["feat"].numpy(), ref["feat"], rtol=1e-12, atol=0)
    for name in cc.layer_names(kind):
        assert np.allclose(got["act." + name].numpy(), ref["act." + name], rtol=1e-12, atol=1e-300), name
        for w in (".weight", ".bias"):
            a, b = got["d." + name + w].numpy(), ref["d." + name + w]
            assert np.abs(b).max() > 0 and np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), name + w


def test_bf16_round_is_nearest_with_ties_to_even():
    one = np.float32(1.0)
    ulp = np.float32(2.0 ** -7)                                       # bf16 spacing in [1, 2)
    x = torch.tensor([one + ulp / 2, one + 3 * ulp / 2, one + ulp / 4, one + 3 * ulp / 4, -(one + ulp / 2), -(one + 3 * ulp / 2),
                      0.0, 3.0e38], dtype=torch.float32)
    want = torch.tensor([one, one + 2 * ulp, one, one + ulp, -one, -(one + 2 * ulp), 0.0, 3.0e38], dtype=torch.float32)
    got = cb.bf16_round(x)
    assert torch.equal(got[:7], want[:7])
    assert got.dtype == torch.float32 and cb.bf16_round(x.double()).dtype == torch.float64
    assert torch.equal(cb.bf16_round(x.double())[:7], want[:7].double())
    r = torch.randn(4096, generator=torch.Generator().manual_seed(1))
    q = cb.bf16_round(r)
    assert torch.equal(cb.bf16_round(q), q)                           # idempotent
    assert bool(((q - r).abs() <= r.abs() * 2.0 ** -8).all())         # within half a unit of 8 significant bits
    assert bool(((q.view(torch.int32) & 0xFFFF) == 0).all())          # the low 16 bits of every result are clear


@pytest.mark.parametrize("kind,B,u8", cb.PARITY_CASES)
def test_every_parity_case_is_nontrivial(kind, B, u8):
    P, d = cc.convstack_params(kind, cb.PARITY_SEED), cc.convstack_data(kind, B, cb.PARITY_SEED, u8=u8)
    res = cb.chain(kind, P, d, torch.float64)
    assert cb.nontrivial(kind, {k: v.numpy() for k, v in res.items()})


@pytest.mark.parametrize("kind", [0, 1])
def test_the_all_bytes_case_is_nontrivial(kind):
    P, d = cb.all_bytes_case(kind)
    res = cb.chain(kind, P, d, torch.float64)
    assert cb.nontrivial(kind, {k: v.numpy() for k, v in res.items()})


def test_the_pool_backward_takes_the_first_maximum_and_drops_non_positive_ones():
    act = torch.tensor([[[[1.0, 1.0, 0.0, 0.0], [0.5, 1.0, 0.0, 0.0], [2.0, 3.0, -0.0, 0.0], [3.0, 1.0, 0.0, 0.0]]]])
    dx = torch.tensor([[[[10.0, 20.0], [30.0, 40.0]]]])
    g = cb.gate_below(dx, act, True)
    want = torch.zeros(1, 1, 4, 4)
    want[0, 0, 0, 0] = 10.0                                           # the first of three equal maxima
    want[0, 0, 2, 1] = 30.0                                           # (the window of zeros drops 20 and 40)
    assert torch.equal(g, want)
    assert torch.equal(cb.gate_below(dx, torch.tensor([[[[1.0, 0.0], [-1.0, 2.0]]]]), False), torch.tensor([[[[10.0, 0.0], [0.0, 40.0]]]]))


def test_workspace_query_of_the_ex_entries():
    import var_amd
    lib = var_amd.load_library()
    for kind in (0, 1, 2):
        for B in (1, 2, 3, 5, 43, 400, 1024):
            old, fp32, bf16 = (lib.var_convstack_workspace_bytes(kind, B), lib.var_convstack_workspace_bytes_ex(kind, B, 0),
                               lib.var_convstack_workspace_bytes_ex(kind, B, 1))
            assert old > 0 and fp32 == old
            assert bf16 >= old and bf16 % 16 == 0
        for flags in (2, 3, 4, -1, 1 << 16):
            assert lib.var_convstack_workspace_bytes_ex(kind, 2, flags) == -1, flags
        for B in (0, -1, 1025):
            assert lib.var_convstack_workspace_bytes_ex(kind, B, 0) == -1 and lib.var_convstack_workspace_bytes_ex(kind, B, 1) == -1
    for kind in (-1, 3):
        assert lib.var_convstack_workspace_bytes_ex(kind, 2, 0) == -1 and lib.var_convstack_workspace_bytes_ex(kind, 2, 1) == -1
    # kind 2 computes in fp32 under the flag: the same workspace
    assert lib.var_convstack_workspace_bytes_ex(2, 7, 1) == lib.var_convstack_workspace_bytes(2, 7)


def test_an_unknown_precision_is_refused_without_a_device():
    import var_amd
    module = cc.stack_module(1, cc.convstack_params(1, 1))
    image = torch.zeros(1, 3, 96, 96)
    for bad in ("fp16", "BF16", None, 1):
        with pytest.raises(var_amd.VarHipError, match="precision"):
            var_amd.conv_stack_eval(module, image, precision=bad)
    with pytest.raises(var_amd.VarHipError, match="precision"):
        var_amd.bind_convs(object(), precision="fp16")

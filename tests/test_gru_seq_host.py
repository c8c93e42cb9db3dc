"""Host-side checks of the PPO update's recurrent sequence (no GPU): the float64 checker of tests/gru_seq_cpu.py reproduces the
fixture made from the reference's NNBase._forward_gru (tests/golden/gru_seq_t7.npz), its two restatements agree, the public
names exist and refuse what they cannot run before any library call; and the faults a third env block and a second M tile can
have, injected into torch's fp32 evaluation standing in for the device, are rejected by the bounds of the shape that first has them."""
import types

import numpy as np
import pytest
import torch
import torch.nn as nn

from tests import gru_seq_cpu as gc


def test_fixture_is_the_shape_and_mask_pattern_the_tests_rely_on(golden_dir):
    d, g = gc.load_fixture(golden_dir)
    T, N, I, H = gc.FIXTURE_SHAPE
    assert d["x"].shape == (T * N, I) and d["hxs"].shape == (N, H) and d["w_ih"].shape == (3 * H, I) and d["w_hh"].shape == (3 * H, H)
    assert g["out"].shape == (T * N, H) and g["h_T"].shape == (N, H) and int(g["seed"]) == 453
    m = d["masks"].reshape(T, N)
    assert set(np.unique(m)) == {0.0, 1.0}
    assert m[0].min() == 0 and m[0].max() == 1 and not m[2].any() and m[3].sum() == N - 1 and m[5].sum() == N - 1 and m[6].min() == 0
    assert np.abs(d["hxs"]).min() > 0 and np.abs(d["b_ih"]).min() > 0 and np.abs(d["b_hh"]).min() > 0
    w = d["w_hh"].astype(np.float64)
    assert np.abs(w.T @ w - np.eye(H)).max() < 1e-5                # orthogonal (model.py:96-100)
    assert np.array_equal(g["h_T"], g["out"][-N:])


@pytest.mark.parametrize("with_dhT", [False, True])
def test_float64_checker_reproduces_the_reference_fixture(golden_dir, with_dhT):
    """float64 against the reference's fp32: 1e-6 relative to each array's largest magnitude."""
    d, g = gc.load_fixture(golden_dir)
    res = gc.evaluate(d, torch.float64, "steps", with_dhT=with_dhT)
    dist = gc.fixture_distances(res, g, with_dhT)
    print("float64 definition vs the reference fixture:", dist)
    assert set(dist) == set(gc.OUTPUTS + gc.GRADS)
    for k, v in dist.items():
        assert v <= 1e-6, (k, v)


@pytest.mark.parametrize("shape", [(1, 1, 4, 64), (4, 3, 20, 64), (7, 5, 128, 512)])
def test_per_step_and_segmented_restatements_agree(golden_dir, shape):
    """In float64 both forms are one function up to the summation order inside torch's GRU cell."""
    d = gc.load_fixture(golden_dir)[0] if shape == gc.FIXTURE_SHAPE else gc.gru_inputs(*shape, seed=5)
    a = gc.evaluate(d, torch.float64, "steps")
    b = gc.evaluate(d, torch.float64, "segmented")
    for k in a:
        assert gc.rel(b[k], a[k]) <= 1e-12, k


def test_zero_mask_cuts_the_history_in_the_checker():
    d = gc.gru_inputs(4, 3, 20, 64, seed=6)
    m = d["masks"].reshape(4, 3)
    m[:] = 1.0
    m[2, 1] = 0.0
    a = gc.evaluate(d, torch.float64, "steps", with_dhT=False)
    e = dict(d)
    e["hxs"] = d["hxs"] + 1.0
    e["x"] = d["x"].copy()
    e["x"].reshape(4, 3, 20)[:2, 1] += 1.0
    b = gc.evaluate(e, torch.float64, "steps", with_dhT=False)
    assert np.array_equal(a["out"].reshape(4, 3, 64)[2:, 1], b["out"].reshape(4, 3, 64)[2:, 1])
    assert not np.array_equal(a["out"].reshape(4, 3, 64)[2:, 0], b["out"].reshape(4, 3, 64)[2:, 0])


def test_public_names_exist():
    import var_amd
    for name in ("masked_gru", "forward_gru", "bind_forward_gru"):
        assert callable(getattr(var_amd, name)), name
    from var_amd._lib import EXPORTED_SYMBOLS
    assert {"var_gru_seq_workspace_bytes", "var_gru_seq_fwd", "var_gru_seq_bwd"} <= set(EXPORTED_SYMBOLS)
    lib = var_amd.load_library()
    assert lib.var_gru_seq_workspace_bytes(100, 4, 128, 512) > 4 * 100 * 4 * 3 * 512
    for bad in ((0, 4, 128, 512), (1, 0, 128, 512), (1, 65, 128, 512), (1, 4, 0, 512), (1, 4, 1025, 512), (1, 4, 128, 96),
                (1, 4, 128, 1088), (1, 4, 128, 0)):
        assert lib.var_gru_seq_workspace_bytes(*bad) == -1, bad


def _args(T=2, N=3, I=8, H=64, **over):
    a = dict(x=torch.zeros(T * N, I), hxs=torch.zeros(N, H), masks=torch.ones(T * N, 1), w_ih=torch.zeros(3 * H, I),
             w_hh=torch.zeros(3 * H, H), b_ih=torch.zeros(3 * H), b_hh=torch.zeros(3 * H))
    a.update(over)
    return [a[k] for k in ("x", "hxs", "masks", "w_ih", "w_hh", "b_ih", "b_hh")]


def test_errors_are_raised_before_any_library_call(monkeypatch):
    import var_amd
    from var_amd import gru_seq

    def boom(*a, **k):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(gru_seq.Context, "get", boom)
    E = var_amd.VarHipError
    with pytest.raises(E, match="CUDA"):
        var_amd.masked_gru(*_args())                               # CPU tensors: no fallback
    meta = lambda args: [t.to("meta") for t in args]               # noqa: E731  (shape / dtype checks need no device)
    with pytest.raises(E):
        var_amd.masked_gru(*meta(_args()))                         # not CUDA either
    # the checks themselves, on tensors that claim to be CUDA tensors of the wrong kind
    chk = gru_seq._check

    class Fake:
        """A stand-in that answers the questions _check asks, so that the shape rules run without a GPU."""
        def __init__(self, t, dtype=None):
            self.t, self.dtype, self.is_cuda, self.device, self.shape = t, dtype or t.dtype, True, "cuda:0", t.shape
        def dim(self):
            return self.t.dim()
        def numel(self):
            return self.t.numel()
    monkeypatch.setattr(gru_seq.torch, "is_tensor", lambda t: True)
    fake = lambda args: [Fake(t) for t in args]                    # noqa: E731
    assert chk(*fake(_args())) == (2, 3, 8, 64)
    assert chk(*fake(_args(T=1))) == (1, 3, 8, 64)
    for bad in (dict(H=96), dict(H=1088), dict(N=65), dict(I=1025), dict(x=torch.zeros(7, 8)), dict(x=torch.zeros(6, 8, 1)),
                dict(masks=torch.ones(5, 1)), dict(masks=torch.ones(3, 2)), dict(w_ih=torch.zeros(192, 9)),
                dict(w_hh=torch.zeros(128, 64)), dict(b_ih=torch.zeros(191)), dict(b_hh=torch.zeros(192, 1)),
                dict(hxs=torch.zeros(3, 64, 1))):
        with pytest.raises(E):
            chk(*fake(_args(**bad)))
    a = fake(_args())
    a[0] = Fake(a[0].t, torch.float64)
    with pytest.raises(E, match="float32"):
        chk(*a)
    a = fake(_args())
    a[4] = Fake(a[4].t, torch.float16)
    with pytest.raises(E, match="float32"):
        chk(*a)


def test_forward_gru_and_binding_refuse_what_they_cannot_run():
    import var_amd
    E = var_amd.VarHipError
    x, hxs, masks = torch.zeros(6, 8), torch.zeros(3, 64), torch.ones(6, 1)
    for gru in (nn.GRU(8, 64, num_layers=2), nn.GRU(8, 64, bidirectional=True), nn.GRU(8, 64, bias=False), nn.LSTM(8, 64), None):
        with pytest.raises(E):
            var_amd.forward_gru(gru, x, hxs, masks)
    with pytest.raises(E):
        var_amd.forward_gru(nn.GRU(8, 64), x, hxs, masks)          # a fine GRU, but CPU tensors
    with pytest.raises(E):
        var_amd.bind_forward_gru(nn.Linear(3, 3))
    with pytest.raises(E):
        var_amd.bind_forward_gru(types.SimpleNamespace(base=types.SimpleNamespace(gru=nn.GRU(8, 64, bidirectional=True))))
    pol = gc.StandInPolicy(8, 64, 2, seed=1)
    assert var_amd.bind_forward_gru(pol) is pol and var_amd.bind_forward_gru(pol.base) is pol.base
    with pytest.raises(E):
        pol.base(x, hxs, masks)                                    # bound: the CPU call now fails loudly


# ---- the shapes that first run a tiling path: that their bounds would notice what the path can get wrong -------------------------
def _stand_in(shape):
    """torch's fp32 CPU evaluation of the segmented form standing in for the device at a GPU case's own inputs."""
    d = gc.gru_inputs(*shape, seed=100 + sum(shape))
    return gc.evaluate(d, torch.float32, "segmented"), gc.evaluate(d, torch.float64, "steps"), gc.gru_bounds(*shape, True)


def test_a_third_env_block_fault_is_rejected_at_33_envs():
    """One env of the third block of 16 (env 32 of 33) given its neighbour's state at every step; no case before had a third block."""
    shape = T, N, I, H = (2, 33, 129, 128)
    assert -(-N // 16) == 3 and -(-17 // 16) == 2                   # (17 envs was the most run before)
    t32, ref, bound = _stand_in(shape)
    out = t32["out"].reshape(T, N, H).copy()
    out[:, 32] = out[:, 31]
    bad = {"out": out.reshape(T * N, H), "h_T": out[-1]}
    for k in gc.OUTPUTS:
        ok, b = gc.rel(t32[k], ref[k]) / bound[k], gc.rel(bad[k], ref[k]) / bound[k]
        print(f"env 32 with env 31's state, {k} at {shape}: sound {ok:.3f} of the bound, the fault {b:.3g} x")
        assert ok <= 1.0 < b, (k, ok, b)


@pytest.mark.parametrize("stale", [0.0, -77.0])
def test_an_unwritten_second_m_tile_is_rejected_at_129_inputs(stale):
    """d_x (rows, I) and d_w_ih (3H, I) are products with M = I on tiles of 128: at I = 129 input 128 is a second tile of one row;
    left unwritten it holds whatever the buffer held.  With I <= 128, all that ran before, there is no second tile."""
    shape = T, N, I, H = (2, 33, 129, 128)
    assert -(-I // 128) == 2 and -(-128 // 128) == 1
    t32, ref, bound = _stand_in(shape)
    for k in ("d_x", "d_w_ih"):
        bad = t32[k].copy()
        bad[:, 128:] = stale
        ok, b = gc.rel(t32[k], ref[k]) / bound[k], gc.rel(bad, ref[k]) / bound[k]
        print(f"input 128 of {k} left at {stale} at {shape}: sound {ok:.3f} of the bound, the fault {b:.3g} x")
        assert ok <= 1.0 < b, (k, ok, b)

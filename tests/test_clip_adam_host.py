"""Host-side checks of the fused PPO optimiser (no GPU): tests/clip_adam_cpu.py's float64 restatement against
torch.nn.utils.clip_grad_norm_ + torch.optim.Adam run in float64, and what var_amd.ClipAdam does before any launch -- its segment
table (pointer arithmetic, so CPU tensors serve), the parameters it leaves out, the gradient set it insists on, and state_dict in
torch.optim.Adam's layout in both directions."""
import ctypes

import numpy as np
import pytest
import torch

from tests import clip_adam_cpu as ca


def close64(a, b, ulps=8):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool(np.all(np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)))))


@pytest.mark.parametrize("norm_ratio", [4.0, 0.25, None])
def test_restatement_equals_torch_in_float64_over_three_steps(norm_ratio):
    """clip64 / clip_adam64 against the real thing in float64, state carried over three steps (planted each step from the
    restatement's own results): equal to a few roundings of double."""
    lens = (1, 3, 64, 257, 1000)
    h0 = ca.carried(ca.hyper(1, None if norm_ratio is None else ca.MAX_NORM))
    inp = ca.inputs(lens, 3, "general", ca.hyper(2), 1.0)
    ps, ms, vs = (ca.split(inp[k].astype(np.float64), lens) for k in "pmv")
    for step in (1, 2, 3):
        h = h0._replace(step=step)
        g = ca.inputs(lens, 10 + step, "general", ca.hyper(2), norm_ratio or 1.0)["g"].astype(np.float64)
        gs = ca.split(g, lens)
        total, coef, out = ca.clip_adam64(ps, gs, ms, vs, h, norm_eps=1e-6)              # (float64 torch adds the double 1e-6)
        tn, tp, tm, tv = ca.clip_adam_torch(ps, gs, ms, vs, h, torch.float64)
        if norm_ratio is None:
            assert total is None and tn is None and coef == 1.0
        else:
            assert close64(total, tn) and (coef < 1.0) == (norm_ratio > 1)
        for (p1, m1, v1, u), a, b, c, p0, m0, g0 in zip(out, tp, tm, tv, ps, ms, gs):
            assert np.all(np.abs(m1 - b) <= 8 * np.spacing(np.abs(m0) + np.abs(g0 * coef)))      # (the scale without cancellation)
            assert close64(v1, c)
            assert np.all(np.abs(p1 - a) <= 8 * np.spacing(np.abs(p0) + np.abs(u)))              # (p' = p - u rounds at p's size)
        ps, ms, vs = [o[0] for o in out], [o[1] for o in out], [o[2] for o in out]


def test_lib_signature_and_segment_struct():
    import var_amd
    from var_amd._lib import EXPORTED_SYMBOLS, OptSeg
    assert "var_clip_adam_step" in EXPORTED_SYMBOLS and hasattr(var_amd.load_library(), "var_clip_adam_step")
    assert ctypes.sizeof(OptSeg) == 40                           # var_opt_seg: four pointers and a long
    assert var_amd.ClipAdam is var_amd.optim.ClipAdam


def arena(sizes, holes=()):
    """Parameters that are consecutive views of one flat tensor (an arena policy's layout), with a gap in front of those in `holes`."""
    flat = torch.zeros(sum(sizes) + 8 * len(holes) + 8)
    ps, o = [], 0
    for i, n in enumerate(sizes):
        if i in holes:
            o += 8
        ps.append(torch.nn.Parameter(flat[o:o + n]))
        o += n
    return flat, ps


def test_table_merges_contiguous_neighbours_and_skips_none_gradients():
    import var_amd
    sizes = (5, 1, 7, 3, 2, 4)
    flat, ps = arena(sizes, holes=(4,))
    opt = var_amd.ClipAdam(ps, lr=1e-3, max_norm=0.5)
    gflat = torch.ones(sum(sizes))
    views, o = [], 0
    for n in sizes:
        views.append(gflat[o:o + n])
        o += n
    # parameters 0..2: gradients from one flat buffer; 3: a gradient of its own; 4 (behind a gap in the arena), 5: one buffer again
    for i, p in enumerate(ps):
        p.grad = views[i] if i != 3 else torch.ones(sizes[3])
    segs, grads = opt._table()
    assert [s[4] for s in segs] == [13, 3, 6] and len(grads) == 6       # 2 | 3: g breaks; 3 | 4: p and g break; 4 | 5: all four go on
    assert segs[0][0] == ps[0].data_ptr() and segs[0][1] == gflat.data_ptr() and segs[0][2] == opt.exp_avg.data_ptr()
    assert segs[2][0] == ps[4].data_ptr() and segs[2][1] == views[4].data_ptr()
    assert segs[2][2] == opt.exp_avg.data_ptr() + 4 * 16 and segs[2][3] == opt.exp_avg_sq.data_ptr() + 4 * 16
    ps[5].grad = torch.ones(sizes[5])                            # 4 | 5: now g alone breaks
    assert [s[4] for s in opt._table()[0]] == [13, 3, 2, 4]
    # a gradient that is not contiguous is made so (and then stands alone)
    opt2 = var_amd.ClipAdam(ps[:2], lr=1e-3)
    ps[0].grad = torch.ones(5, 2)[:, 0]
    ps[1].grad = views[1]
    segs, grads = opt2._table()
    assert [s[4] for s in segs] == [5, 1] and grads[0].is_contiguous() and segs[0][1] == grads[0].data_ptr()
    # parameters without a gradient are left out, and the moments' run breaks there
    flat, ps = arena((4, 4, 4))
    opt3 = var_amd.ClipAdam(ps, lr=1e-3)
    g = torch.ones(12)
    ps[0].grad, ps[2].grad = g[0:4], g[4:8]
    segs, _ = opt3._table()
    assert [s[4] for s in segs] == [4, 4] and segs[1][2] == opt3.exp_avg.data_ptr() + 4 * 8
    assert opt3._active == (0, 2)


def test_a_changed_gradient_set_and_wrong_inputs_are_refused():
    import var_amd
    flat, ps = arena((4, 4, 4))
    opt = var_amd.ClipAdam(ps, lr=1e-3, max_norm=1.0)
    ps[0].grad, ps[1].grad = torch.ones(4), torch.ones(4)
    opt._table()
    opt._table()                                                 # (the same set again: fine)
    ps[2].grad = torch.ones(4)
    with pytest.raises(var_amd.VarHipError, match="differs from the first step"):
        opt._table()
    ps[2].grad, ps[1].grad = None, None
    with pytest.raises(var_amd.VarHipError, match="differs from the first step"):
        opt._table()
    opt.zero_grad()
    assert all(p.grad is None for p in ps)
    with pytest.raises(var_amd.VarHipError, match="GPU only"):
        opt.step()                                               # CPU parameters: no fallback
    fresh = var_amd.ClipAdam(ps, lr=1e-3)
    with pytest.raises(var_amd.VarHipError, match="no parameter has a gradient"):
        fresh._table()
    for bad in (dict(params=[]), dict(params=[torch.zeros(3, dtype=torch.float64)]), dict(params=[ps[0], ps[0]]), dict(betas=(0.9, 1.0)),
                dict(eps=-1.0), dict(max_norm=0.0), dict(max_norm=float("nan")), dict(lr=None)):
        kw = dict(params=ps, lr=1e-3)
        kw.update(bad)
        with pytest.raises(var_amd.VarHipError):
            var_amd.ClipAdam(**kw)


def test_param_groups_serve_update_linear_schedule():
    import var_amd
    _, ps = arena((3, 2))
    opt = var_amd.ClipAdam(ps, lr=6e-5, eps=1e-5, max_norm=0.5)
    assert len(opt.param_groups) == 1 and opt.param_groups[0]["params"] == ps
    assert opt.param_groups[0]["lr"] == 6e-5 and opt.param_groups[0]["betas"] == (0.9, 0.999) and opt.param_groups[0]["eps"] == 1e-5
    for group in opt.param_groups:                               # models/ppo/utils.py:45-49
        group["lr"] = 6e-5 - 6e-5 * (1 / 4.0)
    assert opt.param_groups[0]["lr"] == 4.5e-5 and opt._lr_written == 6e-5         # (reaches the device at the next step())


def test_state_dict_moves_between_clip_adam_and_torch_adam():
    import var_amd
    sizes = (6, 1, 5)
    g = torch.Generator().manual_seed(5)
    _, ps = arena(sizes)
    with torch.no_grad():
        for p in ps:
            p.copy_(torch.randn(p.shape, generator=g))
    ref = torch.optim.Adam(ps, lr=6e-5, eps=1e-5)
    for _ in range(3):
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        ref.step()
    # torch -> ClipAdam
    opt = var_amd.ClipAdam(ps, lr=1.0, eps=1.0, max_norm=0.5)
    opt.load_state_dict(ref.state_dict())
    assert opt.step_count() == 3 and opt._active == (0, 1, 2)
    assert opt.param_groups[0]["lr"] == 6e-5 and opt.param_groups[0]["eps"] == 1e-5 and opt.param_groups[0]["params"] == ps
    o = 0
    for p in ps:
        assert torch.equal(opt.exp_avg[o:o + p.numel()], ref.state[p]["exp_avg"])
        assert torch.equal(opt.exp_avg_sq[o:o + p.numel()], ref.state[p]["exp_avg_sq"])
        o += p.numel()
    # ClipAdam -> torch: a fresh Adam that loads it takes the same next step as the one the state came from
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and set(sd["state"]) == {0, 1, 2} and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    assert set(sd["param_groups"][0]) == set(ref.state_dict()["param_groups"][0])
    _, qs = arena(sizes)
    with torch.no_grad():
        for q, p in zip(qs, ps):
            q.copy_(p)
    other = torch.optim.Adam(qs, lr=1.0)
    other.load_state_dict(opt.state_dict())                      # (its own copy: torch.optim.Adam steps the loaded tensors in place)
    for p, q in zip(ps, qs):
        p.grad = torch.randn(p.shape, generator=g)
        q.grad = p.grad.clone()
    ref.step()
    other.step()
    for p, q in zip(ps, qs):
        assert torch.equal(p, q) and float(other.state[q]["step"]) == 4
    # and back: ClipAdam reads what it wrote; a never-stepped one has no state
    again = var_amd.ClipAdam(ps, lr=1.0)
    again.load_state_dict(sd)
    assert torch.equal(again.exp_avg, opt.exp_avg) and torch.equal(again.exp_avg_sq, opt.exp_avg_sq) and again.step_count() == 3
    assert var_amd.ClipAdam(ps, lr=1.0).state_dict()["state"] == {}
    bad = ref.state_dict()
    bad["state"][1]["step"] = torch.tensor(7.0)
    with pytest.raises(var_amd.VarHipError, match="one step count"):
        var_amd.ClipAdam(ps, lr=1.0).load_state_dict(bad)
    bad = ref.state_dict()
    bad["param_groups"][0]["weight_decay"] = 0.1
    with pytest.raises(var_amd.VarHipError, match="weight decay"):
        var_amd.ClipAdam(ps, lr=1.0).load_state_dict(bad)

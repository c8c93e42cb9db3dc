"""The checker of tests/test_gpu_ithor_reward_layers.py, pinned on the CPU (tests/ithor_reward_layers_cpu.py): chained in float64
its layer functions ARE the frozen encoder's reward step (oracle.torch_oracle.IthorNetCPU in .double() to 1e-12, and the
reference's fixture tests/golden/ithor_h96.npz at tests/test_oracle_ithor.py's tolerance); with torch's fp32 kernels standing in
for the device every row passes on both GRU routes; and each fault a kernel of this kind can have -- injected into ONE buffer,
everything upstream intact, everything downstream computed from it -- fails the rows of that buffer and no other.  For the record
(printed, and tabulated in DESIGN section 7): how far each fault moves image_feat / goal_feat / reward, which is all
tests/test_gpu_ithor_reward.py sees, at atol 1e-4.  No GPU needed."""
import functools
import os

import numpy as np
import pytest
import torch

from oracle.torch_oracle import ithor_seeded
from tests import _ithor_reward_inputs as rin
from tests import ithor_reward_layers_cpu as rl

B, PLAN = 3, 4
OLD_ATOL = 1e-4                    # tests/test_gpu_ithor_reward.py: the embeddings against the checker
ROUTES = ("fused", "split")


@functools.lru_cache(maxsize=None)
def params():
    return {k: v.detach().clone().float() for k, v in rin.spread_checker().state_dict().items()}


def inputs(seed):
    img, snd = rin.spread_inputs(B, seed)
    return torch.from_numpy(img), torch.from_numpy(snd)


@functools.lru_cache(maxsize=None)
def clean(route, seed=21, head=None):
    """(parameters, fp32 chain) of one goal step: torch's fp32 CPU kernels standing in for the device.  `head`: that head's
    last Linear set to zero."""
    torch.set_num_threads(min(16, torch.get_num_threads()))
    P = params() if head is None else rl.zero_head(params(), head)
    with torch.no_grad():
        return P, rl.chain(P, *inputs(seed), route)


@functools.lru_cache(maxsize=None)
def clean_rows(route, head=None):
    """Every row's result on the clean fp32 chain."""
    P, b = clean(route, head=head)
    with torch.no_grad():
        return rl.check_layers(b, P, route)


def test_float64_chain_is_the_model():
    torch.set_num_threads(min(16, torch.get_num_threads()))
    net = rin.spread_checker().double()
    P64 = {k: v.detach() for k, v in net.state_dict().items()}
    img, snd = inputs(21)
    with torch.no_grad():
        want_i = torch.nn.functional.normalize(net.imgTriplet(net.imgBranch(img.double() / 255)), p=2, dim=1)
        sraw = net.sound_raw(snd.double())
        want_g = torch.nn.functional.normalize(net.soundTriplet(sraw), p=2, dim=1)
        for route in ROUTES:
            b = rl.chain(P64, img, snd, route)
            for k, want in (("image_feat", want_i), ("goal_feat", want_g), ("h73", sraw), ("reward", (want_i * want_g).sum(1))):
                assert b[k].dtype == torch.float64 and b[k].shape == want.shape
                assert float((b[k] - want).abs().max()) <= 1e-12, (route, k)
            # and every row holds on the chain's own buffers at float64 round-off
            for r in rl.rows(route):
                Q = rl.params(P64)
                ref = r.fn(*[Q[k] if k in Q else b[k] for k in r.ins])
                assert rl.rel(r.got(b[r.out]) if r.got else b[r.out], ref) <= 1e-12, (route, r.name)
    assert torch.equal(rl.arena_of(P64), torch.cat([p.detach().reshape(-1) for p in net.parameters()]))


def test_float64_chain_matches_the_reference_fixture(golden_dir):
    g = np.load(os.path.join(golden_dir, "ithor_h96.npz"))
    P64 = {k: v.detach().double() for k, v in ithor_seeded(int(g["seed"])).state_dict().items()}
    with torch.no_grad():
        b = rl.chain(P64, torch.from_numpy(g["image"]), torch.from_numpy(g["sound_positive"]), "fused")
    for k, name in (("image_feat", "image_feat"), ("goal_feat", "sound_feat_positive"), ("a6", "image_feat_raw"), ("h73", "pos_sound_raw")):
        np.testing.assert_allclose(b[k].numpy(), g[name], rtol=1e-5, atol=1e-6, err_msg=k)      # (tests/test_oracle_ithor.py's)


@pytest.mark.parametrize("route", ROUTES)
def test_torch_fp32_passes_every_row(route):
    P, b = clean(route)
    with torch.no_grad():
        res = rl.check_layers(b, P, route, log=lambda s: print(f"{route}: {s}"))
        image_only = rl.check_layers(b, P, route, goal=False)
    assert list(res) == [r.name for r in rl.rows(route)] and len(res) == (20 if route == "fused" else 22)
    assert list(image_only) == list(rl.IMAGE_SIDE) + ["reward", "frozen"]
    bad = {k: r for k, r in res.items() if not r[2] <= 1}
    assert not bad, bad
    assert [k for k, r in res.items() if r[1] == 0] == ["frozen"]                       # the one copy: bound 0
    assert ("gh" in b) == (route == "split")


@pytest.mark.parametrize("route", ROUTES)
def test_every_fault_fails_the_rows_of_its_buffer_and_no_other(route):
    other = clean(route, seed=22)[1]
    wrong, kinds = [], set()
    with torch.no_grad():
        table = rl.faults(clean(route)[1], params(), route, other, PLAN)
        for f in table:
            head = None if f.P is None else [h for h in ("imgTriplet.2", "soundTriplet.4") if not f.P[h + ".bias"].any()][0]
            P, b = clean(route, head=head)
            if head:
                assert float(b["image_feat" if head == "imgTriplet.2" else "goal_feat"].abs().max()) == 0      # F.normalize's result
            y = f.value
            assert y.shape == b[f.buffer].shape and not torch.equal(y, b[f.buffer]), f.what
            env = rl.chain(P, None, None, route, start=dict(b, **{f.buffer: y}), changed=[f.buffer])
            # a row is a function of the buffers it reads and the one it checks: where none of them changed, the clean result holds
            moved_bufs = {k for k in env if env[k] is not b[k]}
            touched = [r.name for r in rl.rows(route) if moved_bufs & set(r.ins + [r.out])]
            res = dict(clean_rows(route, head), **rl.check_layers(env, P, route, only=touched))
            failed = tuple(k for k, r in res.items() if not r[2] <= 1)
            # what the output-only tests see: the rest of the step from the faulty buffer, against the clean outputs
            moved = max(rl.rel(env[o], b[o], 1.0) for o in rl.OUTPUTS)                  # (NaN: inf)
            old = "passes" if moved <= OLD_ATOL else "fails"
            worst = min(res[k][2] for k in f.fails)
            print(f"{route:5s} {f.what:50s} {f.buffer:10s} rows {'+'.join(f.fails):18s} {worst:10.3g} x the bound; "
                  f"outputs move {moved:.1e}: {old} at atol {OLD_ATOL}")
            kinds.add(f.what)
            nan = bool(torch.isnan(y).any())           # a NaN is reported by every row downstream of it as well
            if not (set(f.fails) <= set(failed) if nan else failed == f.fails):
                wrong.append((f.what, f.buffer, f.fails, failed))
    assert len(kinds) == (19 if route == "fused" else 21), sorted(kinds)
    assert not wrong, wrong


def test_a_finite_state_read_by_step_0_is_forgotten_after_72_steps():
    """Why the stale-state check of the GPU test fills the slots with NaN: the update gates of this GRU let a finite initial
    state decay below fp32 resolution long before step 72, so no check of h72 can see it; a NaN never decays."""
    P, b = clean("fused")
    Q = rl.params(P)
    with torch.no_grad():
        h = rl.gru_chain(b["gi"].double(), Q["rnn.w_hh"].double(), Q["rnn.b_hh"].double(), h0=torch.full_like(b["h72"], 0.5))
        ref = rl.gru_chain(b["gi"].double(), Q["rnn.w_hh"].double(), Q["rnn.b_hh"].double())
    print("a state of 0.5 at step 0 moves h72 by", float((h - ref).abs().max()))
    assert float((h - ref).abs().max()) < 1e-9


def test_the_order_yardstick_is_the_same_function_and_still_catches_a_fault():
    """The emulation of ORDER's one row (sound conv 2 on one accumulator) computes that row's function at fp32 round-off of the
    float64 one; the clean buffer passes against it, and one output row of a clip the emulation does not run over, missing one
    tap, is far outside MARGIN times its distance."""
    P, b = clean("fused")
    assert set(rl.ORDER) == {("s2", None)} and set(rl.order_for("fused")) == set(rl.order_for("split")) == {"s2"}
    order = rl.order_for("fused")
    with torch.no_grad():
        x, w, c = b["s1"], P["cnn.2.weight"], P["cnn.2.bias"]
        ref = rl.snd2(x.double(), w.double(), c.double())
        d = rl.order_distance(order["s2"], [x, w, c], ref)
        print(f"s2 kernel order {d:.2e}  torch fp32 {rl.rel(rl.snd2(x, w, c), ref):.2e}")
        assert rl.rel(rl.snd2(x, w, c), ref) < d < 2e-6, d
        assert rl.check_layers(b, P, "fused", order=order, only=["s2"])["s2"][2] <= 1
        # output row 60 of the first channel that is alive there (many are dead past the ReLU), MIDDLE clip, tap (ky, kx) = (0, 4)
        w0 = w.clone()
        w0[:, :, 0, 4] = 0
        s2, wrong = b["s2"].clone(), rl.snd2(x, w0, c)
        ch = int(torch.nonzero((wrong[1, :, 60] - s2[1, :, 60]).abs().amax(1))[0])
        s2[1, ch, 60] = wrong[1, ch, 60]
        assert not torch.equal(s2, b["s2"])
        res = rl.check_layers(dict(b, s2=s2), P, "fused", order=order, only=["s2"])
        assert res["s2"][2] > 1e3, res

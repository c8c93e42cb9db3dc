"""Host checks of the env wrapper's device step (csrc/env_step.hip, var_amd/collect.py) that need no GPU: the numpy
restatement of var_reward_norm_step (tests/env_step_cpu.py) against var_amd.ReturnNormalizer and the reference's own numbers
(tests/golden/reward_norm.npz), bit for bit; the two injected faults, which must show; and the segment tables CollectStep builds
for RolloutStorage.insert, against the storage's shapes."""
import functools
import os
import types

import numpy as np
import pytest
import torch

from tests import env_step_cpu as es


def bits(a):
    return np.ascontiguousarray(np.asarray(a, np.float64)).view(np.uint64)


@functools.lru_cache(maxsize=None)
def seq(n):
    return es.sequence(n)


@functools.lru_cache(maxsize=None)
def restated(n, **kw):
    return es.run_restatement(n, seq(n), **kw)


@pytest.mark.parametrize("n", es.NS)
def test_restatement_equals_the_host_normalizer_bit_for_bit(n):
    import var_amd
    assert seq(n)[2][es.ALL_DONE_STEP].all() and not seq(n)[2].all()
    got, want = restated(n), es.run_host_normalizer(var_amd, n, seq(n))
    for k in ("out64", "ret", "rms"):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.array_equal(got["reward"][..., 0], want["out64"].astype(np.float32))
    if n >= 7:
        assert (got["ret"][es.ALL_DONE_STEP] == 0).all() and np.abs(got["ret"]).max() > 0


def test_restatement_reproduces_the_reference_fixture(golden_dir):
    fx = dict(np.load(os.path.join(golden_dir, "reward_norm.npz")))
    T, n = fx["rews"].shape
    for clip, key in ((10.0, "out"), (1.5, "out_clip15")):
        st = es.NormStep(n, cliprew=clip)
        out = np.stack([st(None, fx["rews"][t], fx["news"][t])[4] for t in range(T)])
        assert np.array_equal(bits(out), bits(fx[key])), key
        assert st.rms[0] == fx["mean"] and st.rms[1] == fx["var"] and st.rms[2] == fx["count"]


@pytest.mark.parametrize("n", [9, 17])
@pytest.mark.parametrize("fault", ["pairwise", "zero_first"])
def test_injected_faults_change_an_output(n, fault):
    """The GPU comparison is only worth something if a kernel that sums left to right, or zeroes ret before the update, would
    fail it on these inputs (the seed of env_step_cpu.sequence is chosen so that both show at both sizes)."""
    good = restated(n)
    bad = restated(n, **({"pairwise": False} if fault == "pairwise" else {"zero_first": True}))
    differs = [k for k in ("out64", "ret", "rms") if not np.array_equal(bits(good[k]), bits(bad[k]))]
    print(n, fault, "differs in", differs)
    assert "rms" in differs and "out64" in differs           # the float64 state after some step, and the float64 quotient


def test_no_normalisation_episode_block_and_slot_words():
    n, T = 9, 3
    dot, env, done, bad = seq(n)
    st = es.NormStep(n, normalise=False, num_steps=T)
    run, last, cnt = np.zeros(n), np.zeros(n), np.zeros(n)
    for t in range(8):
        r32, masks, bm, orig, _ = st(dot[t], env[t], done[t], bad[t])
        rews = dot[t].astype(np.float64) + env[t]
        assert np.array_equal(orig, rews) and np.array_equal(r32[:, 0], rews.astype(np.float32))
        assert np.array_equal(masks[:, 0], 1.0 - done[t]) and np.array_equal(bm[:, 0], 1.0 - bad[t])
        assert tuple(st.slot) == ((t + 1) % T, t % T)
        run = run + rews
        last[done[t]], cnt[done[t]] = run[done[t]], cnt[done[t]] + 1
        run[done[t]] = 0
        assert np.array_equal(st.episode, np.stack([run, last, cnt]))
    assert np.array_equal(st.rms, [0.0, 1.0, 1e-4])


# ---- the insert tables ------------------------------------------------------------------------------------------------------
SLOT_ADD = {"recurrent_hidden_states": 1, "actions": 0, "action_log_probs": 0, "value_preds": 0, "rewards": 0, "masks": 1,
            "bad_masks": 1}


def fake_parts(which, N, T, image_dtype=torch.uint8, store_dtype=None):
    """CPU tensors with the shapes of ActStep (policy._step_spec) and RolloutStorage.__init__ for one policy."""
    from var_amd.actor_critic import ArmNetPolicy, IthorNetPolicy
    if which == "arm":
        fake_self = types.SimpleNamespace(dist=types.SimpleNamespace(logstd=types.SimpleNamespace(_bias=None)))
        kind, n, hidden, _, shapes = ArmNetPolicy._step_spec(fake_self, N, image_dtype)
    else:
        kind, n, hidden, _, shapes = IthorNetPolicy._step_spec(types.SimpleNamespace(n_actions=8), N, image_dtype)
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype)   # noqa: E731
    act = types.SimpleNamespace(obs={k: z(*s, dtype=dt) for k, (s, dt) in shapes.items()}, _hout=z(N, hidden), value=z(N, 1),
                                action=z(N, n) if kind == 0 else z(N, 1, dtype=torch.int64), action_log_probs=z(N, 1), masks=z(N, 1))
    sd = store_dtype or image_dtype
    ro = types.SimpleNamespace(
        num_steps=T, num_processes=N,
        obs={k: z(T + 1, N, *s[1:], dtype=sd if len(s) >= 4 else torch.float32) for k, (s, dt) in shapes.items()},
        recurrent_hidden_states=z(T + 1, N, hidden), rewards=z(T, N, 1), value_preds=z(T + 1, N, 1), action_log_probs=z(T, N, 1),
        actions=z(T, N, n) if kind == 0 else z(T, N, 1, dtype=torch.int64), masks=z(T + 1, N, 1), bad_masks=z(T + 1, N, 1))
    return act, ro, z(N, 1), z(N, 1)


@pytest.mark.parametrize("which", ["arm", "ithor"])
def test_insert_tables_match_the_storage(which):
    from var_amd.collect import MAX_SEGS, insert_segments
    N, T = 8, 3
    act, ro, reward, bad_masks = fake_parts(which, N, T)
    table = insert_segments(act, ro, reward, bad_masks)
    assert len(table) == len(act.obs) + 7 <= MAX_SEGS == 16
    stores = dict(ro.obs, **{k: getattr(ro, k) for k in SLOT_ADD})
    ranges = []
    for name, s in table:
        store = stores[name]
        want_add = 1 if name in ro.obs else SLOT_ADD[name]
        rb = store[0, 0].numel() * store.element_size()
        assert s.slot_add == want_add and s.n_slots == T + want_add, name
        assert s.seg.dst == store.data_ptr() and s.dst_slot_stride == N * rb == store[0].numel() * store.element_size(), name
        assert (s.seg.row_bytes, s.seg.n_t, s.seg.src_env_stride, s.seg.dst_env_stride) == (rb, 1, rb, rb), name
        assert s.n_slots <= store.shape[0]                       # every slot the device word may select lies inside the store
        ranges.append((name + ".dst", s.seg.dst, s.seg.dst + s.n_slots * s.dst_slot_stride))
        ranges.append((name + ".src", s.seg.src, s.seg.src + N * rb))
    for i, (na, a0, a1) in enumerate(ranges):
        for nb, b0, b1 in ranges[i + 1:]:
            assert a1 <= b0 or b1 <= a0, (na, nb)
    srcs = {name: s.seg.src for name, s in table}
    assert srcs["masks"] == act.masks.data_ptr() and srcs["recurrent_hidden_states"] == act._hout.data_ptr()
    assert srcs["image"] == act.obs["image"].data_ptr() and srcs["rewards"] == reward.data_ptr()


def test_insert_table_refuses_another_image_dtype_and_other_shapes():
    from var_amd import VarHipError
    from var_amd.collect import insert_segments
    act, ro, reward, bad_masks = fake_parts("arm", 8, 3, torch.uint8, torch.float32)
    with pytest.raises(VarHipError, match="image dtype"):
        insert_segments(act, ro, reward, bad_masks)
    act, ro, reward, bad_masks = fake_parts("ithor", 8, 3)
    ro.num_processes = 7
    with pytest.raises(VarHipError):
        insert_segments(act, ro, reward, bad_masks)
    act, ro, reward, bad_masks = fake_parts("ithor", 8, 3)
    del ro.obs["occupancy"]
    with pytest.raises(VarHipError):
        insert_segments(act, ro, reward, bad_masks)

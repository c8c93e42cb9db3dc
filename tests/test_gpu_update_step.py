"""GPU checks of PPO.capture / var_amd.UpdateStep (update_step.py): a PPO update whose minibatch steps are replayed graphs
against the eager update of a twin policy with identical weights (bind_convs, fused_optimizer=True, fused_head=True), bit for
bit: the parameter arena, exp_avg, exp_avg_sq, the step count, total_norm and the three returned statistics.  Both run the same
kernels on the same inputs in the same order.  Rollouts as test_gpu_convstack's one-update test builds them: 96 x 96 uint8
images, (T, N) = (3, 2) unless a test says otherwise."""
import types

import pytest
import torch

from tests import convstack_cpu as cc
from tests import trunk_cpu as tc

pytestmark = pytest.mark.gpu

N_ACT = {0: 2, 1: 8}                                             # Box(2) | Discrete(8)
LR = 1e-3


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def policy(var_amd, kind, precision="fp32", binder=None):
    Q = cc.policy_params(kind, 9, N_ACT[kind])
    pol = tc.drop_in_policy(kind, 0).to("cuda")
    with torch.no_grad():
        for k, v in pol.named_parameters():
            v.copy_(torch.from_numpy(Q[k]).cuda())
    assert pol._arena_intact()
    return var_amd.bind_convs(pol, precision=precision) if binder is None else binder(pol)


def shapes_of(kind):
    shapes = {'image': (3, 96, 96), 'image_feat': (3,), 'goal_sound_feat': (3,)}
    shapes.update({'occupancy': (1, 9, 9)} if kind else {'robot_pose': (2,)})
    return shapes


def storage(var_amd, kind, T, N):
    n_act = N_ACT[kind]
    space = type("Discrete", (), {"n": n_act})() if kind else type("Box", (), {"shape": (n_act,)})()
    return var_amd.RolloutStorage(T, N, shapes_of(kind), space, tc.hidden(kind), types.SimpleNamespace(RLObsIgnore=[]),
                                  image_dtype=torch.uint8)


def observation(kind, N, g):
    return {k: (torch.randint(0, 256, (N,) + tuple(sh), generator=g, dtype=torch.uint8) if k in ("image", "occupancy")
                else torch.randn((N,) + tuple(sh), generator=g)).cuda() for k, sh in shapes_of(kind).items()}


def fill(ro, kind, seed):
    """A fresh rollout and compute_returns, as test_one_ppo_update_through_bind_convs_changes_the_arena_in_place."""
    T, N, n_act = ro.num_steps, ro.num_processes, N_ACT[kind]
    g = torch.Generator().manual_seed(seed)
    for _ in range(T):
        act = torch.randint(0, n_act, (N, 1), generator=g) if kind else torch.randn(N, n_act, generator=g)
        ro.insert(observation(kind, N, g), (0.5 * torch.randn(N, tc.hidden(kind), generator=g)).cuda(), act.cuda(),
                  (torch.randn(N, 1, generator=g) * 0.3 - 1.5).cuda(), torch.randn(N, 1, generator=g).cuda(),
                  torch.randn(N, 1, generator=g).cuda(), (torch.rand(N, 1, generator=g) < 0.8).float().cuda(), torch.ones(N, 1).cuda())
    ro.compute_returns(torch.randn(N, 1, generator=g).cuda(), True, 0.99, 0.95, True)


def agent_of(var_amd, pol, epochs=2, mb=2, **kw):
    opts = dict(fused_optimizer=True, fused_head=True)
    opts.update(kw)
    return var_amd.PPO(pol, tc.CLIP, epochs, mb, tc.VCOEF, tc.ECOEF, lr=LR, eps=1e-5, max_grad_norm=0.5, **opts)


def twins(var_amd, kind, precision, T, N, epochs=2, mb=2):
    """(storage, captured agent, its UpdateStep, eager agent) over two policies with identical weights."""
    ro = storage(var_amd, kind, T, N)
    fill(ro, kind, 4)
    cap, eag = (agent_of(var_amd, policy(var_amd, kind, precision), epochs, mb) for _ in range(2))
    step = cap.capture(ro)
    assert isinstance(step, var_amd.UpdateStep) and step.precision == precision
    return ro, cap, step, eag


def state(agent):
    torch.cuda.synchronize()
    opt = agent.optimizer
    return {"arena": agent.actor_critic._flat.clone(), "exp_avg": opt.exp_avg.clone(), "exp_avg_sq": opt.exp_avg_sq.clone(),
            "step": opt._step_dev.clone(), "total_norm": opt._norm.clone()}


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def assert_equal(cap, eag, stats_c, stats_e, what):
    sc, se = state(cap), state(eag)
    for k in sc:
        assert same_bits(sc[k], se[k]), (what, k, int((sc[k].view(torch.int32) != se[k].view(torch.int32)).sum()))
    assert tuple(stats_c) == tuple(stats_e), (what, stats_c, stats_e)
    assert all(x == x for x in stats_c) and bool(torch.isfinite(sc["arena"]).all())


def both_update(ro, cap, eag, seed, what, how=None):
    torch.manual_seed(seed)
    stats_c = (how or cap.update)(ro)
    torch.manual_seed(seed)
    stats_e = eag.update(ro)
    assert_equal(cap, eag, stats_c, stats_e, what)
    return stats_c


@pytest.mark.parametrize("kind,precision", [(0, "fp32"), (0, "bf16"), (1, "fp32"), (1, "bf16")])
def test_a_captured_update_equals_the_eager_update(var_amd, kind, precision):
    ro, cap, step, eag = twins(var_amd, kind, precision, 3, 2)
    before = cap.actor_critic._flat.clone()
    assert step.n_graphs == 1
    both_update(ro, cap, eag, 5, f"kind {kind} {precision}")
    assert int(cap.optimizer._step_dev.item()) == 4              # ppo_epoch 2 x num_mini_batch 2
    assert bool((cap.actor_critic._flat != before).any())
    for name, prm in cap.actor_critic.named_parameters():
        assert prm.grad is not None and prm.grad.shape == prm.shape, name


@pytest.mark.parametrize("kind,precision", [(0, "fp32"), (1, "bf16")])
def test_a_short_last_minibatch_has_its_own_graph(var_amd, kind, precision):
    ro, cap, step, eag = twins(var_amd, kind, precision, 2, 5)   # minibatches of 2, 2 and 1 envs
    assert step.n_graphs == 2
    both_update(ro, cap, eag, 6, "short last minibatch")
    assert int(cap.optimizer._step_dev.item()) == 6


def test_run_eager_equals_a_replay(var_amd):
    ro = storage(var_amd, 0, 3, 2)
    fill(ro, 0, 4)
    a, b = (agent_of(var_amd, policy(var_amd, 0)) for _ in range(2))
    sa, sb = a.capture(ro), b.capture(ro)
    torch.manual_seed(7)
    stats_a = sa.update(ro)
    torch.manual_seed(7)
    stats_b = sb.run_eager(ro)
    assert_equal(a, b, stats_a, stats_b, "run_eager")


def test_later_updates_lr_changes_and_eager_steps_need_no_second_capture(var_amd):
    kind = 0
    ro, cap, step, eag = twins(var_amd, kind, "fp32", 3, 2)
    pol = cap.actor_critic
    flat, addr, graphs, buffers = pol._flat, pol._flat.data_ptr(), step.n_graphs, step.buffer_addresses()
    acting = pol.capture(2, deterministic=True)                   # made before any update
    both_update(ro, cap, eag, 5, "first update")
    # a fresh rollout on the same storage
    ro.after_update()
    fill(ro, kind, 8)
    both_update(ro, cap, eag, 9, "second update, fresh rollout")
    # a changed learning rate reaches the replay
    for agent in (cap, eag):
        agent.optimizer.param_groups[0]["lr"] = 0.25 * LR
    both_update(ro, cap, eag, 10, "changed lr")
    # an eager step between two captured updates
    for agent in (cap, eag):
        torch.manual_seed(11)
        sample = next(iter(ro.recurrent_generator(ro.advantages(), 1)))
        total, *_ = agent.loss(sample)
        agent.optimizer.zero_grad()
        total.backward()
        agent.optimizer.step()
    assert_equal(cap, eag, (0.0,), (0.0,), "eager step in between")
    both_update(ro, cap, eag, 12, "captured after eager")
    assert step.n_graphs == graphs and step.buffer_addresses() == buffers and cap._captured is step
    assert pol._flat is flat and flat.data_ptr() == addr and pol._arena_intact()
    for name, prm in pol.named_parameters():
        assert prm.grad is not None, name
    # the acting graph made before the updates acts on the updated weights
    g = torch.Generator().manual_seed(13)
    obs, masks = observation(kind, 2, g), torch.ones(2, 1, device="cuda")
    acting.reset()
    sv, sa, slp, sh = (t.clone() for t in acting(obs, masks))
    v, a, lp, hx = pol.act(obs, torch.zeros(2, tc.hidden(kind), device="cuda"), masks, deterministic=True)
    torch.cuda.synchronize()
    # (test_gpu_act_step.test_deterministic_steps_equal_act's tolerance for a replay: bits, the log-probabilities within 1e-5)
    assert torch.equal(sv, v) and torch.equal(sh, hx) and torch.equal(sa, a) and float((slp - lp).abs().max()) <= 1e-5


def test_capture_and_update_refuse_before_any_launch(var_amd):
    kind = 0
    ro = storage(var_amd, kind, 3, 2)
    fill(ro, kind, 4)
    E = var_amd.VarHipError
    with pytest.raises(E, match="bind_convs"):
        agent_of(var_amd, policy(var_amd, kind, binder=var_amd.bind_trunk)).capture(ro)
    pol = policy(var_amd, kind)
    with pytest.raises(E, match="fused_optimizer"):
        agent_of(var_amd, pol, fused_optimizer=False).capture(ro)
    with pytest.raises(E, match="fused_head"):
        agent_of(var_amd, pol, fused_head=False).capture(ro)
    cpu = types.SimpleNamespace(num_steps=3, num_processes=2, obs={k: torch.zeros(4, 2, *s) for k, s in shapes_of(kind).items()})
    with pytest.raises(E, match="RolloutStorage"):
        agent_of(var_amd, pol).capture(cpu)
    with pytest.raises(E, match="precision"):
        agent_of(var_amd, pol).capture(ro, precision="fp16")
    agent = agent_of(var_amd, pol)
    step = agent.capture(ro)
    before = state(agent)
    other = storage(var_amd, kind, 2, 2)
    fill(other, kind, 4)
    with pytest.raises(E, match="another"):
        step.update(other)
    agent.num_mini_batch = 1
    with pytest.raises(E, match="num_mini_batch"):
        agent.update(ro)
    agent.num_mini_batch = 2
    pol.to("cuda")                                               # (re-flattens: the arena moves)
    with pytest.raises(E, match="moved"):
        agent.update(ro)
    after = state(agent)
    for k in ("exp_avg", "exp_avg_sq", "step", "total_norm"):
        assert same_bits(before[k], after[k]), k
    assert int(after["step"].item()) == 0


def test_the_default_agent_is_unchanged(var_amd):
    """fused_head=False and no capture: two default agents on one seed give equal bits, and fused_head alone changes only which
    launches compute them (the Linear's summation order), not what update() does."""
    kind = 0
    ro = storage(var_amd, kind, 3, 2)
    fill(ro, kind, 4)
    a, b = (agent_of(var_amd, policy(var_amd, kind), fused_head=False) for _ in range(2))
    assert not a.fused_head and getattr(a, "_captured", None) is None
    torch.manual_seed(5)
    stats_a = a.update(ro)
    torch.manual_seed(5)
    stats_b = b.update(ro)
    assert_equal(a, b, stats_a, stats_b, "default agents")

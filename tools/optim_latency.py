#!/usr/bin/env python3
"""Latency of the PPO update's optimiser step (var_amd.ClipAdam; csrc/clip_adam.hip) against what the reference runs there
(models/ppo/algo/ppo.py:89-91: nn.utils.clip_grad_norm_ + optim.Adam) on the same GPU, for the parameter sets of ArmNetPolicy and
IthorNetPolicy with the gradients laid out as PPO.loss(...).backward() through bind_convs leaves them (views of the conv stacks'
and the trunk's flat buffers, the distribution head's own tensors).  Legs, alternating in one process: ClipAdam.step();
clip_grad_norm_ + optim.Adam in PyTorch's default (foreach) form; clip_grad_norm_ + optim.Adam(fused=True).  Then one whole
PPO.update (T = 100, N = 8, ppo_epoch = 1, num_mini_batch = 2: two minibatch steps of 400 rows) with fused_optimizer on and off.
Medians over the runs, three repeats, spread reported; host wall clock around work that ends in a device synchronise.  The
launches of one optimiser step are counted by torch.profiler in a pass of their own, after the timed part.
Writes profiles/optim_latency.json.

usage: python tools/optim_latency.py [--runs 200] [--repeats 3] [--update-runs 10] [--out profiles/optim_latency.json]"""
import argparse
import json
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import var_amd  # noqa: E402
from tools.convstack_latency import make_policy, measure  # noqa: E402
from tools.gru_seq_latency import summarise  # noqa: E402
from tools.trunk_latency import Box, Discrete  # noqa: E402

LR, EPS, MAX_NORM = 6e-5, 1e-5, 0.5                              # RLLr, RLEps, RLMaxGradNorm (Envs/ai2thor/config.py:74-76)
T, N, MB = 100, 8, 2
NAMES = {0: "ArmNetPolicy", 1: "IthorNetPolicy"}


def observations(kind, rows, g):
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)   # noqa: E731
    obs = {"image": torch.randint(0, 256, (rows, 3, 96, 96), device="cuda", generator=g, dtype=torch.uint8), "image_feat": rn(rows, 3),
           "goal_sound_feat": rn(rows, 3)}
    if kind:
        obs["occupancy"] = (torch.rand(rows, 1, 9, 9, device="cuda", generator=g) < 0.3).to(torch.uint8) * 255
    else:
        obs["robot_pose"] = rn(rows, 2)
    return obs


def minibatch(kind, t, n, g):
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)   # noqa: E731
    M = t * n
    masks = torch.ones(t, n, device="cuda")
    masks[0] = 0.0
    act = torch.randint(0, 8, (M, 1), device="cuda", generator=g) if kind else rn(M, 2)
    return (observations(kind, M, g), 0.5 * rn(n, 1024 if kind else 512), act, rn(M, 1), rn(M, 1), masks.view(M, 1), rn(M, 1) - 2.0, rn(M, 1))


def twin_parameters(pol):
    """Copies of the policy's parameters with copies of their gradients, for a torch optimiser of its own."""
    out = []
    for p in pol.parameters():
        q = torch.nn.Parameter(p.detach().clone())
        q.grad = p.grad.detach().clone()
        out.append(q)
    return out


def kernel_launches(fn):
    """Device kernels one call of fn launches, by torch.profiler; None where the profiler gives no device events."""
    from torch.profiler import ProfilerActivity, profile
    try:
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if getattr(e.device_type, "name", "") == "CUDA" and "memcpy" not in e.name.lower()
                 and "memset" not in e.name.lower()]
        return len(names) or None, sorted(set(names))
    except Exception as e:                                       # noqa: BLE001  (a tool: report, do not die after the timed part)
        return None, [f"torch.profiler failed: {e}"]


def filled_rollout(kind, g):
    shapes = {'image': (3, 96, 96), 'image_feat': (3,), 'goal_sound_feat': (3,)}
    shapes.update({'occupancy': (1, 9, 9)} if kind else {'robot_pose': (2,)})
    ro = var_amd.RolloutStorage(T, N, shapes, Discrete() if kind else Box(), 1024 if kind else 512, types.SimpleNamespace(RLObsIgnore=[]),
                                image_dtype=torch.uint8)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)   # noqa: E731
    for _ in range(T):
        obs = observations(kind, N, g)
        act = torch.randint(0, 8, (N, 1), device="cuda", generator=g) if kind else rn(N, 2)
        ro.insert(obs, 0.5 * rn(N, 1024 if kind else 512), act, rn(N, 1) * 0.3 - 1.5, rn(N, 1), rn(N, 1), torch.ones(N, 1, device="cuda"),
                  torch.ones(N, 1, device="cuda"))
    ro.compute_returns(rn(N, 1), True, 0.99, 0.95, True)
    return ro


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--update-runs", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_latency.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []

    def save():
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump({"what": "microseconds per call (host wall clock around work that ends in a device synchronise), medians of `runs` "
                               "alternating calls, `repeats` repeats, spread = largest - smallest median",
                       "runs": a.runs, "repeats": a.repeats, "update_runs": a.update_runs, "lr": LR, "eps": EPS, "max_norm": MAX_NORM,
                       "device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)

    for kind in (0, 1):
        pol = var_amd.bind_convs(make_policy(kind))
        agent = var_amd.PPO(pol, 0.2, 1, MB, 0.5, 0.01, lr=LR, eps=EPS, max_grad_norm=MAX_NORM, fused_optimizer=True)
        agent.optimizer.zero_grad()
        agent.loss(minibatch(kind, 4, N, g))[0].backward()        # the gradients' layout: bind_convs + bind_trunk + the head's own
        opt = agent.optimizer
        segs = len(opt._table()[0])
        legs, opts = {"clip_adam": opt.step}, {}
        for name, kw in (("torch_foreach", {}), ("torch_fused", {"fused": True})):
            params = twin_parameters(pol)
            opts[name] = (params, torch.optim.Adam(params, lr=LR, eps=EPS, **kw))

            def leg(params=params, o=opts[name][1]):
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                o.step()
            legs[name] = leg
        meds = measure(legs, a.runs, a.repeats, warmup=10)
        row = summarise({"what": "optimiser step (gradient clip + Adam)", "policy": NAMES[kind], "tensors": len(list(pol.parameters())),
                         "elements": sum(p.numel() for p in pol.parameters()), "segments": segs}, meds)
        for name in ("torch_foreach", "torch_fused"):
            row[f"ratio_{name}_over_clip_adam"] = row[name + "_us"] / row["clip_adam_us"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        save()
        del legs, opts, opt, agent, pol

    # one whole PPO.update: two minibatch steps of T * N / 2 = 400 rows
    for kind in (0, 1):
        ro = filled_rollout(kind, g)
        agents = {}
        for name, fused in (("fused_optimizer", True), ("torch_optimizer", False)):
            pol = var_amd.bind_convs(make_policy(kind))
            agents[name] = var_amd.PPO(pol, 0.2, 1, MB, 0.5, 0.01, lr=LR, eps=EPS, max_grad_norm=MAX_NORM, fused_optimizer=fused)
        legs = {name: (lambda ag=ag: ag.update(ro)) for name, ag in agents.items()}
        meds = measure(legs, a.update_runs, a.repeats, warmup=2)
        row = summarise({"what": "PPO.update, ppo_epoch 1, num_mini_batch 2 (two minibatch steps)", "policy": NAMES[kind], "T": T, "N": N}, meds)
        row["saved_us_per_minibatch_step"] = (row["torch_optimizer_us"] - row["fused_optimizer_us"]) / MB
        rows.append(row)
        print(json.dumps(row), flush=True)
        save()
        del legs, agents, ro
        torch.cuda.empty_cache()

    # launches of one optimiser step, counted (a pass of its own: tracing slows the host)
    for kind in (0, 1):
        pol = var_amd.bind_convs(make_policy(kind))
        agent = var_amd.PPO(pol, 0.2, 1, MB, 0.5, 0.01, lr=LR, eps=EPS, max_grad_norm=MAX_NORM, fused_optimizer=True)
        agent.optimizer.zero_grad()
        agent.loss(minibatch(kind, 4, N, g))[0].backward()
        counts = {"clip_adam": kernel_launches(agent.optimizer.step)}
        for name, kw in (("torch_foreach", {}), ("torch_fused", {"fused": True})):
            params = twin_parameters(pol)
            o = torch.optim.Adam(params, lr=LR, eps=EPS, **kw)

            def leg(params=params, o=o):
                torch.nn.utils.clip_grad_norm_(params, MAX_NORM)
                o.step()
            counts[name] = kernel_launches(leg)
        segs = len(agent.optimizer._table()[0])
        row = {"what": "kernel launches of one optimiser step (torch.profiler)", "policy": NAMES[kind], "segments": segs,
               "clip_adam_launches_by_rule": 2 * -(-segs // 64)}
        for name, (n, kernels) in counts.items():
            row[name + "_launches"] = n
            if name == "clip_adam" or n is None:
                row[name + "_kernels"] = kernels
        rows.append(row)
        print(json.dumps(row), flush=True)
        save()


if __name__ == "__main__":
    main()

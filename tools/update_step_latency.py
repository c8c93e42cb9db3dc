#!/usr/bin/env python3
"""Latency of one whole PPO.update (ppo_epoch 1, num_mini_batch 2: two minibatch steps) through three routes, for both policies,
fp32 and bf16 convolution stacks, at (T, N) = (100, 8) and (20, 8) -- the small rollout is where a host-bound update would show:
  eager        bind_convs, fused_optimizer=True: the update as it was before the captured step existed (the yardstick)
  fused_head   the same with fused_head=True: the distribution head's Linear inside the loss's call (var_ppo_head_linear)
  captured     PPO.capture(rollouts): every minibatch step one replayed graph (update_step.py)
One process, the legs alternating, host wall clock around an update() that ends in its own host read of the statistics, medians
of `runs` updates, three repeats, spread = largest - smallest median.  Every leg trains its own policy (same initial weights).
Also reported: the device memory the captured step's static buffers hold.  Writes profiles/update_step_latency.json.

usage: python tools/update_step_latency.py [--runs 10] [--repeats 3] [--out profiles/update_step_latency.json]"""
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
from tools.optim_latency import EPS, LR, MAX_NORM, NAMES, observations  # noqa: E402
from tools.trunk_latency import Box, Discrete  # noqa: E402

SHAPES = ((100, 8), (20, 8))
MB = 2


def filled_rollout(kind, T, N, g):
    shapes = {'image': (3, 96, 96), 'image_feat': (3,), 'goal_sound_feat': (3,)}
    shapes.update({'occupancy': (1, 9, 9)} if kind else {'robot_pose': (2,)})
    ro = var_amd.RolloutStorage(T, N, shapes, Discrete() if kind else Box(), 1024 if kind else 512, types.SimpleNamespace(RLObsIgnore=[]),
                                image_dtype=torch.uint8)
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)   # noqa: E731
    for _ in range(T):
        act = torch.randint(0, 8, (N, 1), device="cuda", generator=g) if kind else rn(N, 2)
        ro.insert(observations(kind, N, g), 0.5 * rn(N, 1024 if kind else 512), act, rn(N, 1) * 0.3 - 1.5, rn(N, 1), rn(N, 1),
                  torch.ones(N, 1, device="cuda"), torch.ones(N, 1, device="cuda"))
    ro.compute_returns(rn(N, 1), True, 0.99, 0.95, True)
    return ro


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "update_step_latency.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert a.runs >= 10, "medians of at least 10 updates"
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for T, N in SHAPES:
        for kind in (0, 1):
            ro = filled_rollout(kind, T, N, g)
            for precision in ("fp32", "bf16"):
                agents = {}
                for name, head in (("eager", False), ("fused_head", True), ("captured", True)):
                    pol = var_amd.bind_convs(make_policy(kind), precision=precision)
                    agents[name] = var_amd.PPO(pol, 0.2, 1, MB, 0.5, 0.01, lr=LR, eps=EPS, max_grad_norm=MAX_NORM, fused_optimizer=True,
                                               fused_head=head)
                step = agents["captured"].capture(ro)
                legs = {name: (lambda ag=ag: ag.update(ro)) for name, ag in agents.items()}
                meds = measure(legs, a.runs, a.repeats, warmup=2)
                row = summarise({"what": "PPO.update, ppo_epoch 1, num_mini_batch 2 (two minibatch steps)", "policy": NAMES[kind],
                                 "precision": precision, "T": T, "N": N, "graphs": step.n_graphs,
                                 "captured_static_MiB": step.static_bytes() / 2 ** 20}, meds)
                for name in ("fused_head", "captured"):
                    row[f"ratio_eager_over_{name}"] = row["eager_us"] / row[name + "_us"]
                rows.append(row)
                print(json.dumps(row), flush=True)
                os.makedirs(os.path.dirname(a.out), exist_ok=True)
                with open(a.out, "w") as fh:
                    json.dump({"what": "microseconds per PPO.update (host wall clock around an update that ends in its host read), medians "
                                       "of `runs` alternating updates, `repeats` repeats, spread = largest - smallest median",
                               "runs": a.runs, "repeats": a.repeats, "lr": LR, "eps": EPS, "max_norm": MAX_NORM,
                               "device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)
                del legs, agents, step
                torch.cuda.empty_cache()
            del ro


if __name__ == "__main__":
    main()

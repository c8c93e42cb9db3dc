#!/usr/bin/env python3
"""Host wall clock of one env step of the collection loop at the RL stage's 8 envs, both policies, from "the simulator's
observations are in host arrays" to "the next action is in a host array", two ways in one process:
  (a) what the library offered before CollectStep: IntrinsicReward.step (replayed encoder), the dot read back with .cpu(),
      ReturnNormalizer on the host, reward / masks / bad_masks pushed back up, RolloutStorage.insert, ActStep, action.cpu()
  (b) CollectStep.observe (pinned staging, ONE replay: encoder, var_reward_norm_step, var_rollout_move_at), ActStep with its
      inputs in place, action.cpu()
Steps without a new goal sound (all but the first of an episode).  Each figure is the median of --iters steps, repeated
--repeats times with the legs alternating; the JSON carries the median of the repeats and their spread (max - min), and per
policy whether (b) is no slower than (a) by more than the spread of (a)'s repeats.  Writes profiles/collect_step_latency.json.
    python3 tools/collect_step_latency.py [--envs 8] [--iters 200] [--repeats 3] [--out profiles/collect_step_latency.json]
    rocprofv3 --kernel-trace --stats -d DIR -o collect -f csv -- python3 tools/collect_step_latency.py --replay-only"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_STEPS = 16


class Box:
    shape = (2,)


class Discrete:
    n = 8


def timed(fn, iters, warm=10):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()                                                     # (ends with action.cpu(): the step's one host read)
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return ts[len(ts) // 2]


def build(which, B):
    import numpy as np
    import torch
    import var_amd
    torch.manual_seed(453)
    rng = np.random.default_rng(0)
    if which == "arm":
        enc = var_amd.VARPretextNet(types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 100, 40), representationDim=3))
        cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, robotStateDim=2, RLObsIgnore=[])
        pol = var_amd.ArmNetPolicy(None, Box(), config=cfg, base='arm_VAR', base_kwargs={
            'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 512, 'actionHiddenSize': 128})
        space, frames = Box(), 100
        extras = {'robot_pose': rng.normal(size=(B, 2)).astype(np.float32)}
    else:
        enc = var_amd.IthorVARPretextNet(types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 600, 40), representationDim=3))
        cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, RLObsIgnore=[])
        pol = var_amd.IthorNetPolicy(None, Discrete(), config=cfg, base='ai2thor_VAR', base_kwargs={
            'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 1024, 'actionHiddenSize': 128})
        space, frames = Discrete(), 600
        extras = {'occupancy': ((rng.random((B, 1, 9, 9)) < 0.3) * 255).astype(np.uint8)}
    sim = dict(image=rng.integers(0, 256, size=(B, 3, 96, 96), dtype=np.uint8), extras=extras,
               env_reward=rng.normal(size=B), done=rng.random(B) < 0.1, bad=np.zeros(B, bool),
               goal=rng.normal(size=(B, 1, frames, 40)).astype(np.float32))
    return enc.to("cuda").eval(), pol.to("cuda"), space, cfg, sim


def legs(which, B, replay_only):
    import numpy as np
    import torch
    import var_amd
    enc, pol, space, cfg, sim = build(which, B)
    extra = next(iter(sim["extras"]))
    up = lambda a: torch.from_numpy(a).cuda()                     # noqa: E731
    out = {}

    def storage(act):
        shapes = {k: tuple(v.shape[1:]) for k, v in act.obs.items()}
        return var_amd.RolloutStorage(T_STEPS, B, shapes, space, pol.recurrent_hidden_state_size, cfg, image_dtype=torch.uint8)

    act_b = pol.capture(B, seed=0)
    collect = var_amd.CollectStep(var_amd.IntrinsicReward(enc), act_b, storage(act_b))
    collect.reset(sim["image"], sim["extras"], sim["goal"])

    def leg_b():
        collect.observe(sim["image"], sim["extras"], sim["env_reward"], sim["done"], sim["bad"])
        return act_b(act_b.obs, act_b.masks)[1].cpu()
    out["b_collect_step"] = leg_b
    if replay_only:
        return out

    ir = var_amd.IntrinsicReward(enc).capture(B)
    act_a = pol.capture(B, seed=0)
    ro = storage(act_a)
    norm = var_amd.ReturnNormalizer(B)
    ir.step(up(sim["image"]), up(sim["goal"]))

    def leg_a():
        image = up(sim["image"])
        feat, goal_feat, dot = ir.step(image, None)
        obs = {'image': image, extra: up(sim["extras"][extra]), 'image_feat': feat, 'goal_sound_feat': goal_feat}
        rews = dot.cpu().numpy().astype(np.float64) + sim["env_reward"]          # the blocking read in the middle of the step
        reward = up(norm(rews, sim["done"]).astype(np.float32).reshape(-1, 1))
        masks = up((1.0 - sim["done"]).astype(np.float32).reshape(-1, 1))
        bad_masks = up((1.0 - sim["bad"]).astype(np.float32).reshape(-1, 1))
        ro.insert(obs, act_a._hout, act_a.action, act_a.action_log_probs, act_a.value, reward, masks, bad_masks)
        return act_a(obs, masks)[1].cpu()
    out["a_existing_parts"] = leg_a
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--replay-only", action="store_true", help="only CollectStep + ActStep (for a kernel trace)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "collect_step_latency.json"))
    a = ap.parse_args()
    import torch
    result = {"envs": a.envs, "iters": a.iters, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "unit": "us",
              "what": "host wall clock per env step, observations in host arrays -> action in a host array"}
    for which in ("arm", "ithor"):
        fns = legs(which, a.envs, a.replay_only)
        runs = {k: [] for k in fns}
        for _ in range(a.repeats):
            for k in sorted(fns):
                runs[k].append(timed(fns[k], a.iters))
        r = {k: {"median": round(sorted(v)[len(v) // 2], 1), "spread": round(max(v) - min(v), 1), "repeats": [round(x, 1) for x in v]}
             for k, v in runs.items()}
        if "a_existing_parts" in r:
            ma, mb = r["a_existing_parts"]["median"], r["b_collect_step"]["median"]
            r["b_minus_a"] = round(mb - ma, 1)
            r["a_over_b"] = round(ma / mb, 3)
            r["b_no_slower_than_a_within_the_spread_of_a"] = bool(mb <= ma + r["a_existing_parts"]["spread"])
        result[which] = r
    print(json.dumps(result))
    if not a.replay_only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

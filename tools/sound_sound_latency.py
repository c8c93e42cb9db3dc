#!/usr/bin/env python3
"""Host wall clock of one env step of the collection loop with config.RLRewardSoundSound on, at the RL stage's 8 envs, both
encoders, from "the simulator's observations are in host arrays" to "the next action is in a host array"
(tools/collect_step_latency.py's method and model set-up):
  a_eager_parts        the only way before the captured steps took the term: eager IntrinsicReward.embeddings(image, None,
                       current) (the encoder's forward, three reads back), host IntrinsicReward.reward, ReturnNormalizer,
                       tensors pushed back up, RolloutStorage.insert, ActStep, action.cpu()
  b_collect_step       CollectStep.observe with sound-sound on (ONE replay; no new goal: on iTHOR the current-only step), ActStep
                       with its inputs in place, action.cpu()
  off_collect_step     the control: the same with sound-sound off, tools/collect_step_latency.py's leg (b); compared with the
                       committed profiles/collect_step_latency.json
  iTHOR only:  b_goal_step_merged (observe with a new goal AND the current sound on every step: goal and current clips in one
               16-clip pass) and off_goal_step (sound-sound off, a new goal on every step: the goal-only pass)
Each figure is the median of --iters steps, repeated --repeats times with the legs alternating; the JSON carries the median of
the repeats and their spread (max - min), and per encoder whether (b) is no slower than (a) by more than the spread of (a)'s
repeats.  Writes profiles/sound_sound_latency.json.
    python3 tools/sound_sound_latency.py [--envs 8] [--iters 200] [--repeats 3] [--out profiles/sound_sound_latency.json]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from collect_step_latency import T_STEPS, build, timed  # noqa: E402


def legs(which, B):
    import numpy as np
    import torch
    import var_amd
    enc, pol, space, cfg, sim = build(which, B)
    rng = np.random.default_rng(1)
    current = rng.normal(size=sim["goal"].shape).astype(np.float32)
    extra = next(iter(sim["extras"]))
    up = lambda a: torch.from_numpy(a).cuda()                     # noqa: E731
    out = {}

    def storage(act):
        shapes = {k: tuple(v.shape[1:]) for k, v in act.obs.items()}
        return var_amd.RolloutStorage(T_STEPS, B, shapes, space, pol.recurrent_hidden_state_size, cfg, image_dtype=torch.uint8)

    def collect(sound_sound):
        act = pol.capture(B, seed=0)
        cs = var_amd.CollectStep(var_amd.IntrinsicReward(enc, sound_sound=sound_sound), act, storage(act))
        cs.reset(sim["image"], sim["extras"], sim["goal"])
        return cs, act

    def observe_leg(cs, act, goal, cur):
        def leg():
            cs.observe(sim["image"], sim["extras"], sim["env_reward"], sim["done"], sim["bad"], goal, cur)
            return act(act.obs, act.masks)[1].cpu()
        return leg

    on, act_on = collect(True)                                   # (first: the iTHOR reward plan gets its sound-sound buffers once)
    off, act_off = collect(False)
    out["b_collect_step"] = observe_leg(on, act_on, None, current)
    out["off_collect_step"] = observe_leg(off, act_off, None, None)
    if which == "ithor":
        on2, act_on2 = collect(True)
        off2, act_off2 = collect(False)
        out["b_goal_step_merged"] = observe_leg(on2, act_on2, sim["goal"], current)
        out["off_goal_step"] = observe_leg(off2, act_off2, sim["goal"], None)

    ir = var_amd.IntrinsicReward(enc, sound_sound=True)
    act_a = pol.capture(B, seed=0)
    ro = storage(act_a)
    norm = var_amd.ReturnNormalizer(B)
    ir.embeddings(sim["image"], sim["goal"], current)            # the episode's first step: the goal embedding is cached

    def leg_a():
        image_feat, goal_feat, cur_feat = ir.embeddings(sim["image"], None, current)
        rews = ir.reward(sim["env_reward"], image_feat, goal_feat, cur_feat)[0]
        obs = {'image': up(sim["image"]), extra: up(sim["extras"][extra]), 'image_feat': up(image_feat), 'goal_sound_feat': up(goal_feat)}
        reward = up(norm(rews, sim["done"]).astype(np.float32).reshape(-1, 1))
        masks = up((1.0 - sim["done"]).astype(np.float32).reshape(-1, 1))
        bad_masks = up((1.0 - sim["bad"]).astype(np.float32).reshape(-1, 1))
        ro.insert(obs, act_a._hout, act_a.action, act_a.action_log_probs, act_a.value, reward, masks, bad_masks)
        return act_a(obs, masks)[1].cpu()
    out["a_eager_parts"] = leg_a
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sound_sound_latency.json"))
    a = ap.parse_args()
    import torch
    result = {"envs": a.envs, "iters": a.iters, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "unit": "us",
              "what": "host wall clock per env step with RLRewardSoundSound on, observations in host arrays -> action in a host array"}
    committed = {}
    try:
        with open(os.path.join(ROOT, "profiles", "collect_step_latency.json")) as f:
            committed = json.load(f)
    except OSError:
        pass
    for which in ("arm", "ithor"):
        fns = legs(which, a.envs)
        runs = {k: [] for k in fns}
        for _ in range(a.repeats):
            for k in sorted(fns):
                runs[k].append(timed(fns[k], a.iters))
        r = {k: {"median": round(sorted(v)[len(v) // 2], 1), "spread": round(max(v) - min(v), 1), "repeats": [round(x, 1) for x in v]}
             for k, v in runs.items()}
        ma, mb = r["a_eager_parts"]["median"], r["b_collect_step"]["median"]
        r["b_minus_a"] = round(mb - ma, 1)
        r["a_over_b"] = round(ma / mb, 3)
        r["b_no_slower_than_a_within_the_spread_of_a"] = bool(mb <= ma + r["a_eager_parts"]["spread"])
        r["second_term_costs"] = round(mb - r["off_collect_step"]["median"], 1)
        was = committed.get(which, {}).get("b_collect_step") if committed.get("envs") == a.envs else None
        if was:
            r["off_committed"] = {"median": was["median"], "spread": was["spread"]}
            r["off_minus_committed"] = round(r["off_collect_step"]["median"] - was["median"], 1)
            r["off_within_the_committed_spread"] = bool(abs(r["off_collect_step"]["median"] - was["median"]) <= was["spread"])
        result[which] = r
    print(json.dumps(result))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Host wall clock of one env step of the collection loop with the sounds served from a device clip table, at the RL stage's 8
envs, both encoders, from "the simulator's observations are in host arrays" to "the next action is in a host array"
(tools/sound_sound_latency.py's method and tools/collect_step_latency.py's model set-up):
  a_*   today's CollectStep with feature arrays
          a_ss_step         sound-sound on, no new goal (on iTHOR the current-only sound pass)
          a_ss_goal_step    sound-sound on, a new goal on every step (on iTHOR the merged 16-clip pass)
          a_off_step        sound-sound off, no new goal: the image-only step
          a_off_goal_step   sound-sound off, a new goal on every step
  b_*   CollectStep(..., clip_table=table): the same four steps with clip indices (host int arrays) instead of feature arrays
Each figure is the median of --iters steps, repeated --repeats times with the legs alternating; the JSON carries the median of
the repeats and their spread (max - min), and a_over_b per pair.  table_build: milliseconds per 1000 clips of
IntrinsicReward.build_clip_table from feature arrays and from int16 PCM (host arrays in, table on the device, synchronised;
--build-clips clips, median of the repeats; 1 s clips for the Kuka encoder, 6 s clips for iTHOR).
Writes profiles/clip_table_latency.json.
    python3 tools/clip_table_latency.py [--envs 8] [--iters 200] [--repeats 3] [--out profiles/clip_table_latency.json]
    python3 tools/clip_table_latency.py --replays 200     # no timing: that many id steps per encoder, for a kernel trace"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from collect_step_latency import T_STEPS, build, timed  # noqa: E402

POOL = 64                                                        # clips in the steps' table


def legs(which, B, only_ids=False):
    import numpy as np
    import torch
    import var_amd
    enc, pol, space, cfg, sim = build(which, B)
    rng = np.random.default_rng(1)
    pool = rng.normal(size=(POOL,) + sim["goal"].shape[1:]).astype(np.float32)
    goal_ids, cur_ids = rng.integers(0, POOL, B).astype(np.int32), rng.integers(0, POOL + 1, B).astype(np.int32)
    x = np.concatenate([pool, np.zeros((1,) + pool.shape[1:], np.float32)])
    goal, current = x[goal_ids], x[cur_ids]
    out = {}

    def storage(act):
        shapes = {k: tuple(v.shape[1:]) for k, v in act.obs.items()}
        return var_amd.RolloutStorage(T_STEPS, B, shapes, space, pol.recurrent_hidden_state_size, cfg, image_dtype=torch.uint8)

    def collect(sound_sound, table):
        act = pol.capture(B, seed=0)
        reward = var_amd.IntrinsicReward(enc, sound_sound=sound_sound)
        if table:
            cs = var_amd.CollectStep(reward, act, storage(act), clip_table=reward.build_clip_table(features=pool))
            cs.reset(sim["image"], sim["extras"], goal_ids=goal_ids)
        else:
            cs = var_amd.CollectStep(reward, act, storage(act))
            cs.reset(sim["image"], sim["extras"], goal)
        return cs, act

    def features_leg(cs, act, g, c):
        def leg():
            cs.observe(sim["image"], sim["extras"], sim["env_reward"], sim["done"], sim["bad"], g, c)
            return act(act.obs, act.masks)[1].cpu()
        return leg

    def ids_leg(cs, act, g, c):
        def leg():
            cs.observe(sim["image"], sim["extras"], sim["env_reward"], sim["done"], sim["bad"], goal_ids=g, current_ids=c)
            return act(act.obs, act.masks)[1].cpu()
        return leg

    for name, ss, g in (("ss_step", True, False), ("ss_goal_step", True, True), ("off_step", False, False), ("off_goal_step", False, True)):
        if not only_ids:
            cs, act = collect(ss, False)
            out["a_" + name] = features_leg(cs, act, goal if g else None, current if ss else None)
        cs, act = collect(ss, True)
        out["b_" + name] = ids_leg(cs, act, goal_ids if g else None, cur_ids if ss else None)
    return out


def table_build(which, clips, repeats):
    import numpy as np
    import torch
    import var_amd
    from var_amd.data import synth_clips
    enc = build(which, 8)[0]
    reward = var_amd.IntrinsicReward(enc)
    frames, samples = (100, 16000) if which == "arm" else (600, 96000)
    feats = np.random.default_rng(2).normal(size=(clips, 1, frames, 40)).astype(np.float32)
    pcm = synth_clips(clips, seed=2, n_samples=samples)
    lens = np.full(clips, samples, np.int32)
    r = {}
    for name, kw in (("from_features", dict(features=feats)), ("from_pcm", dict(pcm=pcm, lens=lens))):
        reward.build_clip_table(**kw)                            # warm-up: plans, lazy kernel attributes
        ts = []
        for _ in range(repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reward.build_clip_table(**kw)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3 * 1000.0 / clips)
        r[name] = {"ms_per_1000_clips": round(sorted(ts)[len(ts) // 2], 1), "spread": round(max(ts) - min(ts), 1), "clips": clips,
                   "seconds_per_clip": samples / 16000}
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--build-clips", type=int, default=256)
    ap.add_argument("--replays", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "clip_table_latency.json"))
    a = ap.parse_args()
    import torch
    if a.replays:
        for which in ("arm", "ithor"):
            fns = legs(which, a.envs, only_ids=True)
            for k in sorted(fns):
                for _ in range(a.replays):
                    fns[k]()
        torch.cuda.synchronize()
        return
    result = {"envs": a.envs, "iters": a.iters, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "unit": "us",
              "what": "host wall clock per env step, observations in host arrays -> action in a host array: feature arrays (a_*) "
                      "against clip ids served from a device clip table (b_*)"}
    for which in ("arm", "ithor"):
        fns = legs(which, a.envs)
        runs = {k: [] for k in fns}
        for _ in range(a.repeats):
            for k in sorted(fns):
                runs[k].append(timed(fns[k], a.iters))
        r = {k: {"median": round(sorted(v)[len(v) // 2], 1), "spread": round(max(v) - min(v), 1), "repeats": [round(x, 1) for x in v]}
             for k, v in runs.items()}
        for name in ("ss_step", "ss_goal_step", "off_step", "off_goal_step"):
            r[name + "_a_over_b"] = round(r["a_" + name]["median"] / r["b_" + name]["median"], 3)
        r["ids_ss_step_minus_ids_off_step"] = round(r["b_ss_step"]["median"] - r["b_off_step"]["median"], 1)
        r["table_build"] = table_build(which, a.build_clips, a.repeats)
        result[which] = r
    print(json.dumps(result))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

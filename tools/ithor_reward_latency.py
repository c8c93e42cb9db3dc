#!/usr/bin/env python3
"""The frozen iTHOR encoder's reward step at the RL stage's 8 envs, replayed graphs, one process, legs alternated:
  baseline  var_ithor_encoder_fwd (inference) + var_row_dot, captured the same way -- entries every build has, so this script
            also runs on a build without var_ithor_reward_* and then prints the baseline legs alone;
  new       IntrinsicReward.capture(envs) on the IthorVARPretextNet (var_ithor_reward_step);
each for the image-only step (goal embedding cached) and for the goal step, medians of --iters replays after a warm-up, the
whole set --repeats times (spread = max - min of the medians), and the largest difference between the legs' outputs.
    python3 tools/ithor_reward_latency.py [--envs 8] [--iters 200] [--repeats 3] [--out profiles/ithor_reward_latency.json]
    rocprofv3 --kernel-trace --stats -d DIR -o ir -f csv -- python3 tools/ithor_reward_latency.py --replay-only [new|baseline] [--iters 50]"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, iters, warm=10):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--replay-only", nargs="?", const="new", default=None, choices=("new", "baseline"),
                    help="only the new (default) or only the baseline graphs, --iters replays each (for a kernel trace)")
    a = ap.parse_args()
    import numpy as np
    import torch
    import var_amd
    from var_amd._lib import Context, current_stream_handle, new_graph, ptr
    B = a.envs
    torch.manual_seed(977)
    m = var_amd.IthorVARPretextNet(types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 600, 40), representationDim=3)).to("cuda").eval()
    rng = np.random.default_rng(0)
    img = torch.from_numpy(rng.integers(0, 256, size=(B, 3, 96, 96), dtype=np.uint8)).cuda()
    snd_np = rng.standard_normal((B, 1, 600, 40)).astype(np.float32) * 6.0
    snd_np[:, :, :, 0] += 18.0
    snd = torch.from_numpy(snd_np).cuda()
    c = Context.get(0)
    have_new = hasattr(c.lib, "var_ithor_reward_step")
    legs, outs = {}, {}

    if a.replay_only != "new":
        flat = m.flat_parameters()
        m._ensure_plan(c, B)
        b_if, b_gf, b_rw = (torch.zeros((B, 3), device="cuda"), torch.zeros((B, 3), device="cuda"), torch.zeros((B,), device="cuda"))

        def baseline(with_goal):
            c.check(c.lib.var_ithor_encoder_fwd(c.handle, current_stream_handle(), ptr(flat), ptr(img), 1, img.stride(0),
                                                ptr(snd) if with_goal else None, None, B, 96, ptr(b_if),
                                                ptr(b_gf) if with_goal else None, None, None, None, 0), "var_ithor_encoder_fwd")
            c.check(c.lib.var_row_dot(c.handle, current_stream_handle(), ptr(b_if), ptr(b_gf), B, 3, ptr(b_rw)), "var_row_dot")

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        graphs = {}
        with torch.cuda.stream(side):
            for with_goal in (True, False):
                baseline(with_goal)
                torch.cuda.synchronize()
                g = new_graph()
                with torch.cuda.graph(g, stream=side, capture_error_mode="thread_local"):
                    baseline(with_goal)
                graphs[with_goal] = g
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        legs["baseline_image_only_us"] = graphs[False].replay
        legs["baseline_goal_us"] = graphs[True].replay
        graphs[True].replay(); graphs[False].replay()
        torch.cuda.synchronize()
        outs["baseline"] = [t.cpu().numpy().copy() for t in (b_if, b_gf, b_rw)]

    if have_new and a.replay_only != "baseline":
        r = var_amd.IntrinsicReward(m).capture(B)
        new = [t.cpu().numpy().copy() for t in r.step(img, snd)]
        new = [t.cpu().numpy().copy() for t in r.step(img)]
        outs["new"] = new
        legs["new_image_only_us"] = r._graphs[False].replay
        legs["new_goal_us"] = r._graphs[True].replay

    if a.replay_only:
        if not legs:
            raise SystemExit("nothing to replay: this build has no var_ithor_reward_step")
        res = {"envs": B, "iters": a.iters, "graphs": a.replay_only}
        for name, fn in legs.items():
            res[name] = round(timed(fn, a.iters, warm=0), 1)
        print(json.dumps(res))
        return

    meds = {k: [] for k in legs}
    for _ in range(a.repeats):
        for k, fn in legs.items():                              # alternated: one leg after the other, then again
            meds[k].append(round(timed(fn, a.iters), 1))
    res = {"envs": B, "iters": a.iters, "repeats": a.repeats, "device": torch.cuda.get_device_name(0)}
    for k, v in meds.items():
        res[k] = sorted(v)[len(v) // 2]
        res[k.replace("_us", "_repeats_us")] = v
        res[k.replace("_us", "_spread_us")] = round(max(v) - min(v), 1)
    if "new" in outs and "baseline" in outs:
        res["max_abs_diff_new_vs_baseline"] = max(float(np.abs(x - y).max()) for x, y in zip(outs["new"], outs["baseline"]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

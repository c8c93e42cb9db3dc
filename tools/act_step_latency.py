#!/usr/bin/env python3
"""Per-step latency of Policy.act at the RL stage's 8 envs, both policies (ArmNetPolicy 'arm_VAR', IthorNetPolicy
'ai2thor_VAR'), four ways in one process:
  (a) eager act()                                   -- the forward's C call + torch.distributions
  (b) the forward alone as a replayed graph         -- what tools/ithor_policy_latency.py measures; stops before the sampling
  (c) the body of act() captured with torch.cuda.graph over static buffers (forward, torch.distributions with argument
      validation off -- it synchronises --, a copy of rnn_hxs back into the static input): the best a user could do before
  (d) policy.capture(envs) -> ActStep: forward + var_policy_dist in one graph; d_act_step includes the device copies of obs
      and masks into its static buffers (legs b and c read their inputs in place), d_act_step_inputs_in_place is the same call
      with the inputs already in step.obs / step.masks -- the figure to hold against (b) and (c)
Each figure is the median of --iters calls (host clock around call + synchronise), repeated --repeats times with the legs
alternating; the JSON carries the median of the repeats and their spread (max - min).
--bf16 adds the legs of the acting forwards' bf16 mode (policy.set_acting_precision("bf16") / capture(precision="bf16"):
b_forward_replay_bf16, d_act_step_bf16, d_act_step_inputs_in_place_bf16), alternated with the fp32 legs in the same process under
the same protocol -- the fp32 legs are the yardstick --, and per policy the speed-up of the replayed step and whether the bf16 step
is no slower than the fp32 one by more than the two legs' spread.  Writes profiles/act_step_bf16_latency.json.
    python3 tools/act_step_latency.py [--envs 8] [--iters 200] [--repeats 3] [--bf16] [--out profiles/act_step_latency.json]
    rocprofv3 --kernel-trace --stats -d DIR -o act -f csv -- python3 tools/act_step_latency.py --replay-only [--bf16]
(--replay-only --bf16 replays the steps of both precisions: c3f_kernel / c3b_kernel per layer in one kernel trace)"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e6)
    ts.sort()
    return ts[len(ts) // 2]


def build(which, B):
    import torch
    import var_amd
    torch.manual_seed(453)
    g = torch.Generator().manual_seed(0)
    obs = {'image': torch.randint(0, 256, (B, 3, 96, 96), dtype=torch.uint8, generator=g).cuda()}
    if which == "arm":
        m = var_amd.ArmNetPolicy(None, Box(), config=types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, robotStateDim=2),
                                 base='arm_VAR', base_kwargs={'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 512,
                                                              'actionHiddenSize': 128})
        obs['robot_pose'] = torch.randn(B, 2, generator=g).cuda()
    else:
        m = var_amd.IthorNetPolicy(None, Discrete(), config=types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3),
                                   base='ai2thor_VAR', base_kwargs={'recurrent': True, 'recurrentInputSize': 128,
                                                                    'recurrentSize': 1024, 'actionHiddenSize': 128})
        obs['occupancy'] = ((torch.rand(B, 1, 9, 9, generator=g) < 0.3).to(torch.uint8) * 255).cuda()
    obs['image_feat'], obs['goal_sound_feat'] = torch.randn(B, 3, generator=g).cuda(), torch.randn(B, 3, generator=g).cuda()
    m = m.to("cuda")
    hxs = torch.randn(B, m.recurrent_hidden_state_size, generator=g).cuda() * 0.3
    return m, obs, hxs, torch.ones(B, 1, device="cuda")


def capture(body):
    """body() captured on a side stream after one warm-up call, as the package's own captures are made."""
    import torch
    import var_amd
    graph = var_amd._lib.new_graph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body()
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            body()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    return graph


def legs(which, B, replay_only, bf16=False):
    import torch
    m, obs, hxs, masks = build(which, B)
    out = {}

    def step_legs(precision, tag):
        step = m.capture(B, seed=0, precision=precision)
        for k, v in obs.items():
            step.obs[k].copy_(v)
        step.masks.copy_(masks)
        out["d_act_step" + tag] = lambda: step(obs, masks)
        out["d_act_step_inputs_in_place" + tag] = lambda: step(step.obs, step.masks)

    def forward_leg(precision, tag):
        m.set_acting_precision(precision)                        # (read when the call is captured, not at replay)
        out["b_forward_replay" + tag] = capture(lambda: m._base_forward(obs, hxs, masks)).replay
        m.set_acting_precision("fp32")

    step_legs("fp32", "")
    if bf16:
        step_legs("bf16", "_bf16")
    if replay_only:
        return out
    out["a_eager_act"] = lambda: m.act(obs, hxs, masks)
    forward_leg("fp32", "")
    if bf16:
        forward_leg("bf16", "_bf16")

    def act_body():                                              # act() as it stands + the state fed back
        hxs.copy_(m.act(obs, hxs, masks)[3])
    torch.distributions.Distribution.set_default_validate_args(False)
    try:
        out["c_user_graph_of_act"] = capture(act_body).replay
    except Exception as e:                                       # reported, not hidden: the leg is then missing from the figures
        out["c_user_graph_of_act"] = f"capture failed: {type(e).__name__}: {str(e)[:200]}"
        torch.cuda.synchronize()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--replay-only", action="store_true", help="only the new step's replays (for a kernel trace)")
    ap.add_argument("--bf16", action="store_true", help="add the bf16 legs beside the fp32 ones")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "act_step_bf16_latency.json" if a.bf16 else "act_step_latency.json")
    import torch
    result = {"envs": a.envs, "iters": a.iters, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "unit": "us"}
    for which in ("arm", "ithor"):
        fns = legs(which, a.envs, a.replay_only, a.bf16)
        runs = {k: [] for k in fns}
        for _ in range(a.repeats):
            for k in sorted(fns):
                if callable(fns[k]):
                    runs[k].append(timed(fns[k], a.iters))
        r = {}
        for k, v in runs.items():
            r[k] = ({"median": round(sorted(v)[len(v) // 2], 1), "spread": round(max(v) - min(v), 1), "repeats": [round(x, 1) for x in v]}
                    if v else fns[k])
        med = lambda k: r[k]["median"] if isinstance(r.get(k), dict) else None   # noqa: E731
        if med("b_forward_replay") is not None:
            r["d_minus_b"] = round(med("d_act_step_inputs_in_place") - med("b_forward_replay"), 1)
        if med("c_user_graph_of_act") is not None:
            r["c_minus_d"] = round(med("c_user_graph_of_act") - med("d_act_step_inputs_in_place"), 1)
        if a.bf16:
            for k in ("d_act_step_inputs_in_place", "d_act_step", "b_forward_replay"):
                if med(k) is not None and med(k + "_bf16") is not None:
                    slack = max(r[k]["spread"], r[k + "_bf16"]["spread"])
                    r[k + "_fp32_over_bf16"] = round(med(k) / med(k + "_bf16"), 3)
                    r[k + "_bf16_no_slower_within_spread"] = bool(med(k + "_bf16") <= med(k) + slack)
        result[which] = r
    print(json.dumps(result))
    if not a.replay_only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()

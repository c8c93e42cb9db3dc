#!/usr/bin/env python3
"""iTHOR actor-critic forward (IthorNetPolicy, base 'ai2thor_VAR') at the RL stage's 8 envs: eager act() us, replayed
graph forward us (static buffers, as tests/test_gpu_ithor_policy.py captures it) and the same math as torch-eager
(F.conv2d / F.linear from the state_dict, tests/ithor_policy_cpu.py) on the same GPU, in the same process.
    python3 tools/ithor_policy_latency.py [--envs 8] [--iters 200]
    rocprofv3 --kernel-trace --stats -d DIR -o ip -f csv -- python3 tools/ithor_policy_latency.py --replay-only"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


class Discrete:
    def __init__(self, n):
        self.n = n


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
    ap.add_argument("--replay-only", action="store_true", help="only the replayed graph (for a kernel trace)")
    a = ap.parse_args()
    import torch
    import var_amd
    from tests.ithor_policy_cpu import forward as torch_forward
    B = a.envs
    torch.manual_seed(453)
    m = var_amd.IthorNetPolicy(None, Discrete(8), config=types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3),
                               base='ai2thor_VAR', base_kwargs={'recurrent': True, 'recurrentInputSize': 128,
                                                                'recurrentSize': 1024, 'actionHiddenSize': 128}).to("cuda")
    g = torch.Generator().manual_seed(0)
    obs = {'image': torch.randint(0, 256, (B, 3, 96, 96), dtype=torch.uint8, generator=g).cuda(),
           'occupancy': ((torch.rand(B, 1, 9, 9, generator=g) < 0.3).to(torch.uint8) * 255).cuda(),
           'image_feat': torch.randn(B, 3, generator=g).cuda(), 'goal_sound_feat': torch.randn(B, 3, generator=g).cuda()}
    hxs, masks = torch.randn(B, 1024, generator=g).cuda() * 0.3, torch.ones(B, 1, device="cuda")
    graph = var_amd._lib.new_graph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        m._base_forward(obs, hxs, masks)
        torch.cuda.synchronize()
        with torch.cuda.graph(graph, stream=side):
            m._base_forward(obs, hxs, masks)
    torch.cuda.synchronize()
    replay_us = timed(graph.replay, a.iters)
    if a.replay_only:
        print(json.dumps({"envs": B, "replay_us": round(replay_us, 1)}))
        return
    act_us = timed(lambda: m.act(obs, hxs, masks), a.iters)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    fimg, focc = obs['image'].float() / 255., obs['occupancy'].float() / 255.

    @torch.no_grad()
    def eager():
        return torch_forward(sd, obs['image'].float() / 255., obs['occupancy'].float() / 255., obs['image_feat'],
                             obs['goal_sound_feat'], hxs, masks)
    torch_us = timed(eager, a.iters)
    v, f, lg, h = m._base_forward({**obs, 'image': fimg, 'occupancy': focc}, hxs, masks)
    rv, rf, rlg, rh = eager()
    err = max(float((x - y).abs().max()) for x, y in ((v, rv), (f, rf), (lg, rlg), (h, rh)))
    print(json.dumps({"envs": B, "act_us": round(act_us, 1), "replay_us": round(replay_us, 1),
                      "torch_eager_us": round(torch_us, 1), "max_abs_diff_vs_torch": err,
                      "device": torch.cuda.get_device_name(0)}))


if __name__ == "__main__":
    main()

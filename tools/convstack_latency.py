#!/usr/bin/env python3
"""Latency of the actor-critics' convolution stacks (var_amd.conv_stack_eval; csrc/convstack.hip), forward + backward, against
the same nn.Sequential under PyTorch autograd (MIOpen) on the same GPU with the same d_feat: kind 0 (arm_VAR imgCNN) at B = 400
(the reference's update shape, T x N = 100 x 4) and 200, kind 1 (ai2thor_VAR imgCNN) at B = 200, kind 2 (the occupancy
convolutions) at B = 200.  Then PPO.loss(...).backward() of a Kuka ArmNetPolicy at (T, N) = (100, 4) with bind_trunk (stacks
under PyTorch autograd) against bind_convs (stacks in HIP).  One process, both legs warmed up first (MIOpen's solver search stays
outside the timed part), the legs alternating; medians over the runs, three repeats, spread reported.  Host wall clock around
work that ends in a device synchronise.  Writes profiles/convstack_latency.json.

usage: python tools/convstack_latency.py [--runs 30] [--repeats 3] [--out profiles/convstack_latency.json] [--only-hip]
           [--configs 0:400,...]
(--only-hip runs the new op alone, three iterations per shape: the run to put under rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import statistics
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import var_amd  # noqa: E402
from tools.gru_seq_latency import summarise, timed  # noqa: E402
from tools.trunk_latency import Box  # noqa: E402

CONFIGS = ((0, 400), (0, 200), (1, 200), (2, 200))
T, N = 100, 4
# multiply-adds of one image's forward, from the layer shapes (x 2 FLOP; the backward's two products per layer double it again,
# less the first layer's data gradient)
MACS = {0: 96 * 96 * (27 * 32 + 288 * 32) + 48 * 48 * (288 * 64 + 576 * 64) + 24 * 24 * (576 * 128 + 1152 * 128) + 25 * 1152 * 256
        + 9 * 2304 * 128,
        1: 96 * 96 * (27 * 32 + 288 * 32) + 48 * 48 * 288 * 64 + 24 * 24 * 576 * 64 + 12 * 12 * 576 * 128 + 9 * 1152 * 128,
        2: 25 * 9 * 64 + 9 * 576 * 32}


def make_policy(kind):
    kw = {'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 1024 if kind else 512, 'actionHiddenSize': 128}
    torch.manual_seed(0)
    if kind:
        from tools.trunk_latency import Discrete
        cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3)
        pol = var_amd.IthorNetPolicy(None, Discrete(), config=cfg, base='ai2thor_VAR', base_kwargs=kw)
    else:
        cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, robotStateDim=2)
        pol = var_amd.ArmNetPolicy(None, Box(), config=cfg, base='arm_VAR', base_kwargs=kw)
    pol = pol.to("cuda")
    with torch.no_grad():
        for name, prm in pol.named_parameters():                  # (the default initialisation lets the maps fade through eight layers)
            if prm.dim() == 4:
                prm.normal_(0.0, (2.0 / (9 * prm.shape[1])) ** 0.5)
            elif prm.dim() == 1:
                prm.normal_(0.0, 0.1)
    return pol


def measure(legs, runs, repeats, warmup=3):
    for _ in range(warmup):
        for fn in legs.values():
            fn()
    meds = {k: [] for k in legs}
    for _ in range(repeats):
        times = {k: [] for k in legs}
        for _ in range(runs):
            for k, fn in legs.items():
                times[k].append(timed(fn))
        for k in legs:
            meds[k].append(statistics.median(times[k]))
    return meds


def agreement(names, ga, gb):
    worst = max((float((u - v).abs().max() / v.abs().max()), n) for n, u, v in zip(names, ga, gb))
    return {"max_rel_difference": worst[0], "array": worst[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convstack_latency.json"))
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--configs", default=",".join(f"{k}:{b}" for k, b in CONFIGS), help="kind:B,... (default: all)")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    pols = {0: make_policy(0), 1: make_policy(1)}
    g = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for kind, B in (tuple(int(v) for v in c.split(":")) for c in a.configs.split(",")):
        base = pols[1 if kind else 0].base
        module = base.occupancyCNNMLP if kind == 2 else base.imgCNN
        torch_module = torch.nn.Sequential(*list(module)[:5]) if kind == 2 else module
        params = var_amd.convstack.stack_parameters(module)
        shape = (B, 1, 9, 9) if kind == 2 else (B, 3, 96, 96)
        image = torch.randint(0, 256, shape, device="cuda", generator=g, dtype=torch.uint8)
        if kind == 2:
            image = (image < 77).to(torch.uint8) * 255
        d_feat = torch.randn(B, 288 if kind == 2 else 1152, device="cuda", generator=g)

        def hip():
            return torch.autograd.grad((var_amd.conv_stack_eval(module, image) * d_feat).sum(), params)

        def torch_autograd():
            return torch.autograd.grad((torch_module(image.float() / 255.0) * d_feat).sum(), params)

        if a.only_hip:
            for _ in range(3):
                hip()
            torch.cuda.synchronize()
            continue
        names = var_amd.convstack.stack_param_names(kind)
        agree = agreement(names, hip(), torch_autograd())
        meds = measure({"hip": hip, "torch": torch_autograd}, a.runs, a.repeats)
        row = summarise({"what": "conv_stack_eval forward + backward", "kind": kind, "B": B, "gradient_agreement": agree,
                         "forward_gflop": 2e-9 * MACS[kind] * B}, meds)
        row["ratio_torch_over_hip"] = row["torch_us"] / row["hip_us"]
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.only_hip:
        return
    # PPO.loss(...).backward() at the Kuka update shape, stacks under PyTorch autograd (bind_trunk) against in HIP (bind_convs)
    pol, M = pols[0], T * N
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)   # noqa: E731
    obs = {"image": torch.randint(0, 256, (M, 3, 96, 96), device="cuda", generator=g, dtype=torch.uint8), "image_feat": rn(M, 3),
           "goal_sound_feat": rn(M, 3), "robot_pose": rn(M, 2)}
    masks = torch.ones(T, N, device="cuda")
    masks[0] = 0.0
    sample = (obs, 0.5 * rn(N, 512), rn(M, 2), rn(M, 1), rn(M, 1), masks.view(M, 1), rn(M, 1) - 2.0, rn(M, 1))
    agent = var_amd.PPO(pol, 0.2, 1, 1, 0.5, 0.01, lr=1e-4, eps=1e-5, max_grad_norm=0.5)
    binders = {"bind_convs": var_amd.bind_convs, "bind_trunk": var_amd.bind_trunk}

    def leg(name):
        def fn():
            binders[name](pol)                                     # (re-binding swaps one bound method: no device work)
            agent.optimizer.zero_grad()
            agent.loss(sample)[0].backward()
        return fn

    legs = {k: leg(k) for k in binders}
    grads = {}
    for k, fn in legs.items():
        fn()
        grads[k] = [p.grad.clone() for p in pol.parameters()]
    agree = agreement([n for n, _ in pol.named_parameters()], grads["bind_convs"], grads["bind_trunk"])
    meds = measure(legs, a.runs, a.repeats)
    row = summarise({"what": "PPO.loss(sample)[0].backward(), arm_VAR", "T": T, "N": N, "gradient_agreement": agree}, meds)
    row["ratio_bind_trunk_over_bind_convs"] = row["bind_trunk_us"] / row["bind_convs_us"]
    print(json.dumps(row), flush=True)
    rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"what": "microseconds per call (host wall clock around work that ends in a device synchronise), medians of `runs` "
                           "alternating calls, `repeats` repeats, spread = largest - smallest median",
                   "runs": a.runs, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

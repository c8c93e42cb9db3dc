#!/usr/bin/env python3
"""Latency of the PPO update's MLP trunk (var_amd.trunk_eval; csrc/trunk.hip), forward + backward, against the same trunk in
PyTorch autograd on the same GPU, at the reference's update shapes: (T, N) = (100, 4) for arm_VAR (Kuka) and (50, 4) for
ai2thor_VAR (iTHOR), i.e. ppoNumSteps x RLNumEnvs / ppoNumMiniBatch rows.  The PyTorch leg runs twice: with the recurrent sequence
on var_amd.masked_gru (bind_forward_gru: the best the package offered before the trunk op) and with the reference's segmented
torch.nn.GRU (host read of the zero steps included; three interior episode ends).  One process, the legs alternating; medians of
200 runs, three repeats, spread reported; plus the captured-graph replay of the new op (forward + backward as one graph).
Writes profiles/trunk_latency.json.

usage: python tools/trunk_latency.py [--runs 200] [--repeats 3] [--out profiles/trunk_latency.json] [--only-hip]
(--only-hip runs the new op alone, a few iterations: the run to put under rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import var_amd  # noqa: E402
from tools.gru_seq_latency import segmented, summarise, timed  # noqa: E402

CONFIGS = ((0, 100, 4), (1, 50, 4))


class Box:
    shape = (2,)


class Discrete:
    n = 8


def make_base(kind):
    kw = {'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 1024 if kind else 512, 'actionHiddenSize': 128}
    torch.manual_seed(0)
    if kind:
        cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3)
        pol = var_amd.IthorNetPolicy(None, Discrete(), config=cfg, base='ai2thor_VAR', base_kwargs=kw)
    else:
        cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, robotStateDim=2)
        pol = var_amd.ArmNetPolicy(None, Box(), config=cfg, base='arm_VAR', base_kwargs=kw)
    return pol.to("cuda").base


def torch_trunk(base, kind, gru_fn, feat, motor_in, sound_in, hxs, masks, occ):
    """The reference's forward behind imgCNN, module by module (models/RL/arm_RL_model.py:114-134, ai2thor_RL_model.py:90-115)."""
    flat = base.cnnMlp(feat)
    x = flat + base.motorMlp(motor_in)
    if kind:
        for mod in list(base.occupancyCNNMLP)[5:]:
            occ = mod(occ)
        x = x + occ
    g, h_T = gru_fn(base.gru, base.imgMotorMlp(x), hxs, masks)
    y = base.mlp_all(base.fusionMlp(base.soundMlp(sound_in) + flat) + base.imgMotorMlp2(g))
    return base.critic_linear(base.critic(y)), base.actor(y), h_T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "trunk_latency.json"))
    ap.add_argument("--only-hip", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rows = []
    for kind, T, N in CONFIGS:
        base = make_base(kind)
        M, H = T * N, base.gru.hidden_size
        params = var_amd.trunk.trunk_parameters(base)
        with torch.no_grad():
            for prm in params:
                if prm.dim() == 1:
                    prm.normal_(0.0, 0.1)                         # (zero biases would leave half the first layers' units dead)
        g = torch.Generator(device="cuda").manual_seed(1)
        rn = lambda *s: torch.randn(*s, device="cuda", generator=g)   # noqa: E731
        feat = torch.relu(rn(M, 1152)).requires_grad_()
        occ = torch.relu(rn(M, 288)).requires_grad_() if kind else None
        motor_in, sound_in = rn(M, 3 if kind else 5), rn(M, 3)
        hxs = (0.5 * rn(N, H)).requires_grad_()
        masks = torch.ones(T, N, device="cuda")
        masks[0] = 0.0                                            # a rollout's first step after a reset
        for e in range(3):
            masks[(e + 1) * T // 4, e % N] = 0.0                  # three interior episode ends
        masks = masks.view(M, 1)
        d_value, d_feats, d_hT = rn(M, 1), rn(M, 128), rn(N, H)
        leaves = [feat, hxs] + ([occ] if kind else []) + params

        def objective(value, feats, h_T):
            return torch.autograd.grad((value * d_value).sum() + (feats * d_feats).sum() + (h_T * d_hT).sum(), leaves)

        def hip():
            return objective(*var_amd.trunk_eval(base, feat, motor_in, sound_in, hxs, masks, occ=occ))

        def torch_hip_gru():
            return objective(*torch_trunk(base, kind, var_amd.forward_gru, feat, motor_in, sound_in, hxs, masks, occ))

        def torch_nn_gru():
            return objective(*torch_trunk(base, kind, segmented, feat, motor_in, sound_in, hxs, masks, occ))

        if a.only_hip:
            for _ in range(5):
                hip()
            torch.cuda.synchronize()
            continue
        # agreement of the legs' gradients: per leg the worst array (relative to its largest magnitude), and how many of that array's
        # elements are off by more than 1e-4 of it -- a ReLU gate that falls the other way between two summation orders moves a few
        # elements by per cent (tests/trunk_cpu.py), a wrong kernel moves them all
        names = ["d_feat", "d_hxs"] + (["d_occ"] if kind else []) + ["d." + n for n in var_amd.trunk.trunk_param_names(kind)]
        ga, agree = hip(), {}
        for leg, fn in (("torch_hip_gru", torch_hip_gru), ("torch_nn_gru", torch_nn_gru)):
            worst = max(((float((u - v).abs().max() / v.abs().max()), n, int(((u - v).abs() > 1e-4 * v.abs().max()).sum()), v.numel())
                         for n, u, v in zip(names, ga, fn())))
            agree[leg] = {"max_rel_difference": worst[0], "array": worst[1], "elements_off_by_1e-4": worst[2], "elements": worst[3]}
        graph = var_amd._lib.new_graph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(graph, stream=side):
            static = hip()
        torch.cuda.current_stream().wait_stream(side)
        legs = {"hip": hip, "torch_hip_gru": torch_hip_gru, "torch_nn_gru": torch_nn_gru, "hip_graph": graph.replay}
        for _ in range(10):
            for fn in legs.values():
                fn()
        meds = {k: [] for k in legs}
        for _ in range(a.repeats):
            times = {k: [] for k in legs}
            for _ in range(a.runs):
                for k, fn in legs.items():
                    times[k].append(timed(fn))
            for k in legs:
                meds[k].append(statistics.median(times[k]))
        row = summarise({"kind": kind, "T": T, "N": N, "H": H, "interior_episode_ends": 3, "gradient_agreement": agree}, meds)
        row["ratio_vs_torch_hip_gru"] = row["torch_hip_gru_us"] / row["hip_us"]
        row["ratio_vs_torch_nn_gru"] = row["torch_nn_gru_us"] / row["hip_us"]
        row["ratio_graph_vs_torch_hip_gru"] = row["torch_hip_gru_us"] / row["hip_graph_us"]
        del static
        print(json.dumps(row), flush=True)
        rows.append(row)
    if a.only_hip:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"what": "forward + backward of the PPO update's MLP trunk, microseconds per call (host wall clock, synchronised)",
                   "runs": a.runs, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Latency of the actor-critics' convolution stacks (var_amd.conv_stack_eval; csrc/convstack.hip), forward + backward, against
the same nn.Sequential under PyTorch autograd (MIOpen) on the same GPU with the same d_feat: kind 0 (arm_VAR imgCNN) at B = 400
(the reference's update shape, T x N = 100 x 4) and 200, kind 1 (ai2thor_VAR imgCNN) at B = 200, kind 2 (the occupancy
convolutions) at B = 200.  Then PPO.loss(...).backward() of a Kuka ArmNetPolicy at (T, N) = (100, 4) with bind_trunk (stacks
under PyTorch autograd) against bind_convs (stacks in HIP).  One process, both legs warmed up first (MIOpen's solver search stays
outside the timed part), the legs alternating; medians over the runs, three repeats, spread reported.  Host wall clock around
work that ends in a device synchronise.  Writes profiles/convstack_latency.json.

--bf16 adds a third leg beside the two, conv_stack_eval(precision="bf16") / bind_convs(policy, precision="bf16"), alternated with
them in the same process (the yardstick is the fp32 conv_stack_eval leg), and then records the mode's effect on PPO at (T, N) =
(100, 4) for both policies with tests/convstack_cpu.policy_params weights: |ratio - 1| of the importance ratio when the old
log-probabilities come from the fp32 evaluation (which stands for the fp32 acting forward) and the new ones from the bf16
evaluation, and each gradient array's distance from the fp32 leg's; next to that fp32 stand-in row, two pairings with REAL acting
output on the same observations: the log-probabilities policy.act leaves at acting precision "fp32" and at "bf16"
(policy.set_acting_precision; rows of N observations through the acting forward, the rollout's hidden states) against the bf16
evaluation of the same actions.  Writes profiles/convstack_bf16_latency.json.

usage: python tools/convstack_latency.py [--runs 30] [--repeats 3] [--out profiles/convstack_latency.json] [--only-hip]
           [--configs 0:400,...] [--bf16]
(--only-hip runs the new op alone, three iterations per shape: the run to put under rocprofv3 --kernel-trace --stats; with --bf16
it runs the bf16 leg alone)"""
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


def ppo_effect(kind, seed=9):
    """What bf16 evaluation does to the first minibatch after a rollout at (T, N) = (100, 4): max and mean |ratio - 1| with the old
    log-probabilities from the fp32 evaluation of the same minibatch, and every gradient array's distance from the fp32 leg's
    (largest absolute difference over the fp32 array's largest magnitude).  Weights: tests/convstack_cpu.policy_params."""
    from tests import convstack_cpu as cc
    from tests import trunk_cpu as tc
    n_act = 8 if kind else 2
    Q = cc.policy_params(kind, seed, n_act)
    pol = tc.drop_in_policy(kind, 0).to("cuda")
    with torch.no_grad():
        for k, v in pol.named_parameters():
            v.copy_(torch.from_numpy(Q[k]).cuda())
    g = torch.Generator(device="cuda").manual_seed(seed)
    M = T * N
    rn = lambda *s: torch.randn(*s, device="cuda", generator=g)   # noqa: E731
    obs = {"image": torch.randint(0, 256, (M, 3, 96, 96), device="cuda", generator=g, dtype=torch.uint8), "image_feat": rn(M, 3),
           "goal_sound_feat": rn(M, 3)}
    if kind:
        obs["occupancy"] = (torch.rand(M, 1, 9, 9, device="cuda", generator=g) < 0.3).to(torch.uint8) * 255
    else:
        obs["robot_pose"] = rn(M, 2)
    masks = torch.ones(T, N, device="cuda")
    masks[0] = 0.0
    hxs = 0.5 * rn(N, tc.hidden(kind))
    logp, actions = {}, None
    with torch.no_grad():
        for prec in ("fp32", "bf16"):
            var_amd.bind_convs(pol, precision=prec)
            _value, feats, _h, _ = pol.base(obs, hxs, masks.view(M, 1), infer=False)
            if kind:                                               # Categorical over the logits / DiagGaussian (models/ppo/distributions.py)
                lsm = torch.log_softmax(pol.dist.linear(feats), dim=-1)
                if actions is None:
                    actions = torch.multinomial(lsm.exp(), 1, generator=g)
                logp[prec] = lsm.gather(1, actions)
            else:
                mean, logstd = pol.dist.fc_mean(feats), pol.dist.logstd._bias.view(1, -1)
                if actions is None:
                    actions = mean + logstd.exp() * rn(M, n_act)
                logp[prec] = (-0.5 * ((actions - mean) / logstd.exp()) ** 2 - logstd - 0.9189385332046727).sum(-1, keepdim=True)
    ratio = torch.exp(logp["bf16"] - logp["fp32"])
    acting = acting_pairings(kind, pol, obs, hxs, masks, actions, logp["bf16"], n_act)
    sample = (obs, hxs, actions, rn(M, 1), rn(M, 1), masks.view(M, 1), logp["fp32"], rn(M, 1))
    agent = var_amd.PPO(pol, 0.2, 1, 1, 0.5, 0.01, lr=1e-4, eps=1e-5, max_grad_norm=0.5)
    grads = {}
    for prec in ("fp32", "bf16"):
        var_amd.bind_convs(pol, precision=prec)
        agent.optimizer.zero_grad()
        agent.loss(sample)[0].backward()
        grads[prec] = {n: p.grad.clone() for n, p in pol.named_parameters()}
    dist_g = {n: float((grads["bf16"][n] - v).abs().max() / v.abs().max()) for n, v in grads["fp32"].items()}
    return {"what": "effect of bf16 evaluation on the first PPO minibatch after a rollout", "kind": kind, "T": T, "N": N,
            "max_abs_ratio_minus_1": float((ratio - 1).abs().max()), "mean_abs_ratio_minus_1": float((ratio - 1).abs().mean()),
            "acting_log_probabilities_against_bf16_evaluation": acting,
            "gradient_distance_from_fp32": dist_g, "largest_gradient_distance": max(dist_g.values())}


def acting_pairings(kind, pol, obs, hxs, masks, actions, logp_eval, n_act):
    """|ratio - 1| of the first minibatch when the old log-probabilities are what the ACTING forward computes (the real entry, N
    rows per call, hidden state carried and masked as in the rollout) at acting precision fp32 (the pairing before the acting
    forwards had a bf16 mode) and bf16 (set_acting_precision("bf16")), the new ones from the bf16 evaluation."""
    out = {}
    with torch.no_grad():
        for prec in ("fp32", "bf16"):
            pol.set_acting_precision(prec)
            h, logps = hxs, []
            for t in range(T):
                rows = slice(t * N, (t + 1) * N)
                _value, _feats, head, h = pol._base_forward({k: v[rows] for k, v in obs.items()}, h, masks[t].view(N, 1))
                a = actions[rows]
                if kind:
                    logps.append(torch.log_softmax(head, dim=-1).gather(1, a))
                else:
                    logstd = pol.dist.logstd._bias.view(1, -1)
                    logps.append((-0.5 * ((a - head) / logstd.exp()) ** 2 - logstd - 0.9189385332046727).sum(-1, keepdim=True))
            r = torch.exp(logp_eval - torch.cat(logps))
            out[prec + "_acting"] = {"max_abs_ratio_minus_1": float((r - 1).abs().max()), "mean_abs_ratio_minus_1": float((r - 1).abs().mean())}
        pol.set_acting_precision("fp32")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--only-hip", action="store_true")
    ap.add_argument("--configs", default=",".join(f"{k}:{b}" for k, b in CONFIGS), help="kind:B,... (default: all)")
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "convstack_bf16_latency.json" if a.bf16 else "convstack_latency.json")
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

        def hip_bf16():
            return torch.autograd.grad((var_amd.conv_stack_eval(module, image, precision="bf16") * d_feat).sum(), params)

        if a.only_hip:
            for _ in range(3):
                (hip_bf16 if a.bf16 else hip)()
            torch.cuda.synchronize()
            continue
        names = var_amd.convstack.stack_param_names(kind)
        agree = agreement(names, hip(), torch_autograd())
        legs = {"hip": hip, "torch": torch_autograd}
        if a.bf16:
            legs["hip_bf16"] = hip_bf16
        meds = measure(legs, a.runs, a.repeats)
        row = summarise({"what": "conv_stack_eval forward + backward", "kind": kind, "B": B, "gradient_agreement": agree,
                         "forward_gflop": 2e-9 * MACS[kind] * B}, meds)
        row["ratio_torch_over_hip"] = row["torch_us"] / row["hip_us"]
        if a.bf16:
            row["bf16_gradient_distance_from_fp32"] = agreement(names, hip_bf16(), hip())
            row["ratio_hip_over_hip_bf16"] = row["hip_us"] / row["hip_bf16_us"]
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
    if a.bf16:
        binders["bind_convs_bf16"] = lambda p: var_amd.bind_convs(p, precision="bf16")

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
    if a.bf16:
        row["ratio_bind_convs_over_bind_convs_bf16"] = row["bind_convs_us"] / row["bind_convs_bf16_us"]
    print(json.dumps(row), flush=True)
    rows.append(row)
    if a.bf16:
        for kind in (0, 1):
            row = ppo_effect(kind)
            print(json.dumps(row), flush=True)
            rows.append(row)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"what": "microseconds per call (host wall clock around work that ends in a device synchronise), medians of `runs` "
                           "alternating calls, `repeats` repeats, spread = largest - smallest median",
                   "runs": a.runs, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

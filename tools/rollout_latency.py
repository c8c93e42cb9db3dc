#!/usr/bin/env python3
"""Latency of the device-resident PPO rollout (var_amd.RolloutStorage / ppo_loss; csrc/rollout.hip) against the same steps
written as the reference writes them in torch (models/ppo/storage.py, models/ppo/algo/ppo.py:39-41, 66-87 -- restated here),
on one GPU, T = 100 steps x N = 8 envs, both action kinds.  One process, the two legs of a pair alternating; medians of 200
runs, three repeats, spread reported.  Pairs: insert; compute_returns + advantages; one full set of recurrent minibatches
(num_mini_batch = 2); the loss forward + backward on one 400-row minibatch (head and value are leaf tensors: no network).
Writes profiles/rollout_latency.json.

usage: python tools/rollout_latency.py [--runs 200] [--repeats 3] [--out profiles/rollout_latency.json]"""
import argparse
import json
import os
import statistics
import sys
import time
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import var_amd  # noqa: E402

T, N, MB, HID = 100, 8, 2, 1024
GAMMA, LAMBDA, CLIP, VCOEF, ECOEF = 0.99, 0.95, 0.1, 0.5, 0.01
OBS = {'image': (3, 96, 96), 'occupancy': (1, 9, 9), 'image_feat': (3,), 'goal_sound_feat': (3,)}


class Discrete:
    n = 8


class Box:
    shape = (2,)


# ---- the reference's formulation, restated -------------------------------------------------------------------------------------
def torch_insert(ro, step, obs, hxs, act, logp, value, reward, masks, bad):
    for k in ro.obs:
        ro.obs[k][step + 1].copy_(obs[k])
    ro.recurrent_hidden_states[step + 1].copy_(hxs)
    ro.actions[step].copy_(act)
    ro.action_log_probs[step].copy_(logp)
    ro.value_preds[step].copy_(value)
    ro.rewards[step].copy_(reward)
    ro.masks[step + 1].copy_(masks)
    ro.bad_masks[step + 1].copy_(bad)


def torch_returns(ro, next_value):
    ro.value_preds[-1] = next_value
    gae = 0
    for step in reversed(range(T)):
        delta = ro.rewards[step] + GAMMA * ro.value_preds[step + 1] * ro.masks[step + 1] - ro.value_preds[step]
        gae = delta + GAMMA * LAMBDA * ro.masks[step + 1] * gae
        gae = gae * ro.bad_masks[step + 1]
        ro.returns[step] = gae + ro.value_preds[step]
    adv = ro.returns[:-1] - ro.value_preds[:-1]
    return (adv - adv.mean()) / (adv.std() + 1e-5)


def torch_minibatches(ro, adv):
    per = N // MB
    perm = torch.randperm(N)
    out = []
    for start in range(0, N, per):
        cols = {k: [] for k in list(ro.obs) + ["h", "a", "v", "r", "m", "l", "adv"]}
        for off in range(per):
            ind = perm[start + off]
            for k in ro.obs:
                cols[k].append(ro.obs[k][:-1, ind])
            cols["h"].append(ro.recurrent_hidden_states[0:1, ind])
            cols["a"].append(ro.actions[:, ind]); cols["v"].append(ro.value_preds[:-1, ind])
            cols["r"].append(ro.returns[:-1, ind]); cols["m"].append(ro.masks[:-1, ind])
            cols["l"].append(ro.action_log_probs[:, ind]); cols["adv"].append(adv[:, ind])
        mb = {k: torch.stack(v, 1) for k, v in cols.items()}
        out.append({k: (v.view(per, -1) if k == "h" else v.view(T * per, *v.shape[2:])) for k, v in mb.items()})
    return out


def torch_loss(kind, head, logstd, values, actions, old, adv, ret, vp):
    if kind == 0:
        dist = torch.distributions.Normal(head, (torch.zeros_like(head) + logstd.t().view(1, -1)).exp(), validate_args=False)
        logp = dist.log_prob(actions).sum(-1, keepdim=True)
    else:
        dist = torch.distributions.Categorical(logits=head, validate_args=False)
        logp = dist.log_prob(actions.squeeze(-1)).view(actions.size(0), -1).sum(-1).unsqueeze(-1)
    ent = dist.entropy().mean()
    ratio = torch.exp(logp - old)
    action_loss = -torch.min(ratio * adv, torch.clamp(ratio, 1.0 - CLIP, 1.0 + CLIP) * adv).mean()
    vpc = vp + (values - vp).clamp(-CLIP, CLIP)
    value_loss = 0.5 * torch.max((values - ret).pow(2), (vpc - ret).pow(2)).mean()
    return value_loss * VCOEF + action_loss - ent * ECOEF


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def pair(name, hip, ref, runs, repeats):
    for _ in range(10):
        hip(); ref()
    meds = {"hip": [], "torch": []}
    for _ in range(repeats):
        a, b = [], []
        for _ in range(runs):
            a.append(timed(hip)); b.append(timed(ref))
        meds["hip"].append(statistics.median(a)); meds["torch"].append(statistics.median(b))
    row = {"step": name}
    for k, v in meds.items():
        row[k + "_us"] = statistics.median(v)
        row[k + "_spread_us"] = max(v) - min(v)
    row["ratio"] = row["torch_us"] / row["hip_us"]
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rollout_latency.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    cfg = types.SimpleNamespace(RLObsIgnore=[])
    g = torch.Generator().manual_seed(0)
    rows = []
    for kind, space, n in ((0, Box(), 2), (1, Discrete(), 8)):
        ro = var_amd.RolloutStorage(T, N, OBS, space, HID, cfg, image_dtype=torch.uint8)
        obs = {k: (torch.randint(0, 256, (N, *s), dtype=torch.uint8, generator=g) if len(s) == 3 else torch.randn(N, *s, generator=g)).cuda()
               for k, s in OBS.items()}
        f = lambda *s: torch.randn(*s, generator=g).cuda()        # noqa: E731
        act = f(N, n) if kind == 0 else torch.randint(0, n, (N, 1), generator=g).cuda()
        feed = (obs, f(N, HID), act, f(N, 1) * 0.3 - 1.5, f(N, 1), f(N, 1), torch.ones(N, 1).cuda(), torch.ones(N, 1).cuda())
        for _ in range(T):
            ro.insert(*feed)
        nv = f(N, 1)
        tag = "gaussian" if kind == 0 else "categorical"
        rows.append(pair(f"insert/{tag}", lambda: ro.insert(*feed), lambda: torch_insert(ro, ro.step, *feed), a.runs, a.repeats))
        rows.append(pair(f"returns+advantages/{tag}", lambda: ro.compute_returns(nv, True, GAMMA, LAMBDA, True),
                         lambda: torch_returns(ro, nv), max(a.runs // 10, 5), a.repeats))
        adv = ro.advantages()
        rows.append(pair(f"minibatches/{tag}", lambda: list(ro.recurrent_generator(adv, MB)), lambda: torch_minibatches(ro, adv),
                         a.runs, a.repeats))
        mb = next(iter(ro.recurrent_generator(adv, MB)))
        M = T * N // MB
        head, values = f(M, n).requires_grad_(), f(M, 1).requires_grad_()
        logstd = (torch.zeros(n, 1).cuda().requires_grad_()) if kind == 0 else None

        def hip_loss():
            total = var_amd.ppo_loss(head, logstd, values, mb[2], mb[6], mb[7], mb[4], mb[3], kind=kind, clip_param=CLIP,
                                     value_loss_coef=VCOEF, entropy_coef=ECOEF)[0]
            head.grad = values.grad = None
            total.backward()

        def ref_loss():
            total = torch_loss(kind, head, logstd, values, mb[2], mb[6], mb[7], mb[4], mb[3])
            head.grad = values.grad = None
            total.backward()
        rows.append(pair(f"loss fwd+bwd/{tag}", hip_loss, ref_loss, a.runs, a.repeats))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"T": T, "N": N, "num_mini_batch": MB, "runs": a.runs, "repeats": a.repeats,
                   "device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

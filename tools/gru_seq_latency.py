#!/usr/bin/env python3
"""Latency of the PPO update's recurrent sequence (var_amd.masked_gru; csrc/gru_seq.hip), forward + backward, against the
reference's formulation on the same GPU -- the zero-step search with its host read, one torch.nn.GRU (MIOpen) call per segment,
torch.cat, autograd (models/ppo/model.py:116-171, restated here) -- at the two reference configurations, (T, N, I, H) =
(100, 4, 128, 512) and (50, 4, 128, 1024), with no interior zero mask and with three interior episode ends.  One process, the
two legs alternating; medians of 200 runs, three repeats, spread reported; plus the captured-graph replay of the new op
(forward + backward as one graph).  Writes profiles/gru_seq_latency.json.

usage: python tools/gru_seq_latency.py [--runs 200] [--repeats 3] [--out profiles/gru_seq_latency.json] [--only-hip]
(--only-hip runs the new op alone, a few iterations: the run to put under rocprofv3 --kernel-trace --stats)"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import var_amd  # noqa: E402

CONFIGS = ((100, 4, 128, 512), (50, 4, 128, 1024))


def segmented(gru, x, hxs, masks):
    """NNBase._forward_gru's multi-step branch, host read included."""
    N = hxs.size(0)
    T = x.size(0) // N
    x = x.view(T, N, x.size(1))
    masks = masks.view(T, N)
    has_zeros = (masks[1:] == 0.0).any(dim=-1).nonzero().squeeze().cpu()
    has_zeros = [has_zeros.item() + 1] if has_zeros.dim() == 0 else (has_zeros + 1).numpy().tolist()
    has_zeros = [0] + has_zeros + [T]
    hxs = hxs.unsqueeze(0)
    outputs = []
    for i in range(len(has_zeros) - 1):
        a, b = has_zeros[i], has_zeros[i + 1]
        scores, hxs = gru(x[a:b], hxs * masks[a].view(1, -1, 1))
        outputs.append(scores)
    return torch.cat(outputs, dim=0).view(T * N, -1), hxs.squeeze(0)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6


def summarise(row, meds):
    for k, v in meds.items():
        row[k + "_us"] = statistics.median(v)
        row[k + "_spread_us"] = max(v) - min(v)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gru_seq_latency.json"))
    ap.add_argument("--only-hip", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    rows = []
    for T, N, I, H in CONFIGS:
        for ends in (0, 3):
            torch.manual_seed(0)
            gru = nn.GRU(I, H).cuda()
            for name, prm in gru.named_parameters():
                if "weight" in name:
                    nn.init.orthogonal_(prm)
            params = list(gru.parameters())
            x = torch.randn(T * N, I, device="cuda", requires_grad=True)
            hxs = torch.randn(N, H, device="cuda", requires_grad=True)
            masks = torch.ones(T, N, device="cuda")
            masks[0] = 0.0                                          # a rollout's first step after a reset
            for e in range(ends):
                masks[(e + 1) * T // (ends + 1), e % N] = 0.0
            masks = masks.view(T * N, 1)
            d_out, d_hT = torch.randn(T * N, H, device="cuda"), torch.randn(N, H, device="cuda")
            leaves = [x, hxs] + params

            def hip():
                out, h = var_amd.forward_gru(gru, x, hxs, masks)
                return torch.autograd.grad((out * d_out).sum() + (h * d_hT).sum(), leaves)

            def ref():
                out, h = segmented(gru, x, hxs, masks)
                return torch.autograd.grad((out * d_out).sum() + (h * d_hT).sum(), leaves)

            if a.only_hip:
                for _ in range(5):
                    hip()
                torch.cuda.synchronize()
                continue
            ga, gb = hip(), ref()
            agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(ga, gb))
            graph = var_amd._lib.new_graph()
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.graph(graph, stream=side):
                static = hip()
            torch.cuda.current_stream().wait_stream(side)
            for _ in range(10):
                hip(); ref(); graph.replay()
            meds = {"hip": [], "torch": [], "hip_graph": []}
            for _ in range(a.repeats):
                ta, tb, tc = [], [], []
                for _ in range(a.runs):
                    ta.append(timed(hip)); tb.append(timed(ref)); tc.append(timed(graph.replay))
                meds["hip"].append(statistics.median(ta)); meds["torch"].append(statistics.median(tb))
                meds["hip_graph"].append(statistics.median(tc))
            row = summarise({"T": T, "N": N, "I": I, "H": H, "interior_episode_ends": ends, "segments": ends + 1,
                             "max_rel_gradient_difference": agree}, meds)
            row["ratio"] = row["torch_us"] / row["hip_us"]
            row["ratio_graph"] = row["torch_us"] / row["hip_graph_us"]
            del static
            print(json.dumps(row), flush=True)
            rows.append(row)
    if a.only_hip:
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump({"what": "forward + backward of the masked GRU sequence, microseconds per call (host wall clock, synchronised)",
                   "runs": a.runs, "repeats": a.repeats, "device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Host wall clock of the one-rank replayed Kuka in-batch step (VARTrainer.capture_inbatch_epoch_steps: gather, MFCC, encoder,
head, backward, Adam and row fetch in ONE graph) with the head's three treatments of the candidates of an anchor's own class:
negatives = "all" (the label-blind head, var_inbatch_loss_fwd_bwd), "other_class" and "multi_positive"
(var_inbatch_loss_fwd_bwd_ex with the pool's class tables, gathered inside the graph by the step's index row).
One process, one trainer and one captured graph per leg over the same pool (B = 256, 84 x 84, 4096 triplets), the legs
alternating; each figure is the host clock around --steps replays ending in a synchronise, divided by --steps, after --warmup
replays of every leg; --repeats figures per leg show the spread.  The JSON carries per leg the median, the spread (max - min)
and the repeats, and the two class-aware legs' medians minus "all"'s.  Writes profiles/inbatch_classes_latency.json.
    python3 tools/inbatch_classes_latency.py [--steps 200] [--repeats 5] [--warmup 50] [--out profiles/inbatch_classes_latency.json]
    python3 tools/inbatch_classes_latency.py --replays 200    # no timing: that many replays per leg, for a kernel trace"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEGS = ("all", "other_class", "multi_positive")


def build(batch, hw, pool_items, rows):
    import torch
    import var_amd
    cfg = types.SimpleNamespace(img_dim=(3, hw, hw), sound_dim=(1, 100, 40), representationDim=3)
    pool = var_amd.SyntheticTripletPool(pool_items, hw=hw, seed=0, clips_per_class=64).freeze_pairs()
    table = pool.index_table(batch, rows)[:rows].contiguous()
    out = {}
    for name in LEGS:
        torch.manual_seed(453)
        model = var_amd.VARPretextNet(cfg).to("cuda")
        tr = var_amd.VARTrainer(model, lr=1e-4, weight_decay=1e-6)
        kw = {} if name == "all" else dict(classes=pool.class_tables(), negatives=name)
        replay, _ = tr.capture_inbatch_epoch_steps(pool.images, pool.clips, batch, table, tau=0.1, clip_len=pool.clip_len, **kw)
        out[name] = (tr, replay)
    return pool, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--hw", type=int, default=84)
    ap.add_argument("--pool", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--replays", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "inbatch_classes_latency.json"))
    a = ap.parse_args()
    import torch
    pool, legs = build(a.batch, a.hw, a.pool, 256)
    if a.replays:
        for name in LEGS:
            for _ in range(a.replays):
                legs[name][1]()
        torch.cuda.synchronize()
        return
    for name in LEGS:
        for _ in range(a.warmup):
            legs[name][1]()
    torch.cuda.synchronize()
    runs = {name: [] for name in LEGS}
    for _ in range(a.repeats):
        for name in LEGS:
            replay = legs[name][1]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                replay()
            torch.cuda.synchronize()
            runs[name].append((time.perf_counter() - t0) * 1e3 / a.steps)
    losses = {name: float(legs[name][0].loss.item()) for name in LEGS}
    assert all(x == x and abs(x) < 1e6 for x in losses.values()), losses
    result = {"what": "host wall clock per replayed one-rank Kuka in-batch step (one graph launch), by the head's treatment of the "
                      "candidates of an anchor's own class", "unit": "ms", "batch": a.batch, "hw": a.hw, "pool": a.pool,
              "candidates": 2 * a.batch, "steps": a.steps, "repeats": a.repeats, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0)}
    for name, v in runs.items():
        result[name] = {"median": round(sorted(v)[len(v) // 2], 4), "spread": round(max(v) - min(v), 4),
                        "repeats": [round(x, 4) for x in v], "last_loss": round(losses[name], 4)}
    for name in LEGS[1:]:
        result[name + "_minus_all"] = round(result[name]["median"] - result["all"]["median"], 4)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()

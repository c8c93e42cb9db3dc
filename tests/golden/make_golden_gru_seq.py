#!/usr/bin/env python3
"""Golden vectors for the PPO update's recurrent sequence, made by IMPORTING the reference's models.ppo.model.NNBase on the CPU
and calling its _forward_gru (model.py:116-171) under torch autograd.

T = 7 steps, N = 5 envs, I = 128, H = 512, torch.manual_seed(453): NNBase's own orthogonal weights (model.py:96-100), then small
random non-zero biases, a non-zero hxs; masks with a zero at t = 0, every env zero at t = 2, single zeros at t = 3 and t = 5 and
a zero at the last step.

gru_seq_t7.npz            x, hxs, masks, b_ih, b_hh, d_out, d_hT; out, h_T; the gradients of sum(out * d_out) as g0.* and of
                          sum(out * d_out) + sum(h_T * d_hT) as g1.*: d_x, d_hxs, d_b_ih, d_b_hh in full.  The two weight
                          gradients (3 MB and 0.8 MB) as every 16th row (.rows16) plus the float64 sums along both axes
                          (.rowsum: every row is covered, .colsum).
gru_seq_t7_w_ih.npz       w_ih (1536, 128)
gru_seq_t7_w_hh<k>.npz    rows 384 k .. 384 k + 383 of w_hh (1536, 512), k = 0..3 -- a committed file stays below 1 MiB

usage: make_golden_gru_seq.py REFERENCE_CHECKOUT
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
T, N, I, H, SEED = 7, 5, 128, 512, 453
ROWS = 16


def main(reference):
    sys.path.insert(0, reference)
    torch.set_num_threads(1)
    from models.ppo.model import NNBase
    torch.manual_seed(SEED)
    base = NNBase(True, I, H, 128)
    gru = base.gru
    with torch.no_grad():
        gru.bias_ih_l0.copy_(0.1 * torch.randn(3 * H))
        gru.bias_hh_l0.copy_(0.1 * torch.randn(3 * H))
    x = torch.randn(T * N, I, requires_grad=True)
    hxs = (0.5 * torch.randn(N, H)).requires_grad_()
    masks = torch.ones(T, N)
    masks[0, 0] = 0.0
    masks[2, :] = 0.0
    masks[3, 1] = 0.0
    masks[5, 4] = 0.0
    masks[6, 2] = 0.0
    masks = masks.view(T * N, 1)
    d_out, d_hT = torch.randn(T * N, H), torch.randn(N, H)
    out, h_T = base._forward_gru(x, hxs, masks)
    assert out.shape == (T * N, H) and h_T.shape == (N, H) and float(hxs.abs().min()) > 0
    leaves = [x, hxs, gru.weight_ih_l0, gru.weight_hh_l0, gru.bias_ih_l0, gru.bias_hh_l0]
    names = ("d_x", "d_hxs", "d_w_ih", "d_w_hh", "d_b_ih", "d_b_hh")
    main_npz = {"x": x, "hxs": hxs, "masks": masks, "b_ih": gru.bias_ih_l0, "b_hh": gru.bias_hh_l0, "d_out": d_out, "d_hT": d_hT,
                "out": out, "h_T": h_T, "seed": torch.tensor(SEED)}
    for tag, obj in (("g0.", (out * d_out).sum()), ("g1.", (out * d_out).sum() + (h_T * d_hT).sum())):
        for name, g in zip(names, torch.autograd.grad(obj, leaves, retain_graph=True)):
            if name in ("d_w_ih", "d_w_hh"):
                main_npz[tag + name + ".rows16"] = g[::ROWS]
                main_npz[tag + name + ".rowsum"] = g.double().sum(1)
                main_npz[tag + name + ".colsum"] = g.double().sum(0)
            else:
                main_npz[tag + name] = g
    files = {"gru_seq_t7.npz": main_npz, "gru_seq_t7_w_ih.npz": {"w_ih": gru.weight_ih_l0}}
    for k in range(4):
        files[f"gru_seq_t7_w_hh{k}.npz"] = {"w_hh": gru.weight_hh_l0[384 * k:384 * (k + 1)]}
    for name, content in files.items():
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **{k: v.detach().numpy().copy() for k, v in content.items()})
        size = os.path.getsize(path)
        assert size < (1 << 20), (name, size)
        print(path, size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1])

#!/usr/bin/env python3
"""Golden vectors for the actor-critics' convolution stacks, made by IMPORTING the reference's models.ppo.model.Policy for both
bases ('arm_VAR', Kuka configuration; 'ai2thor_VAR', iTHOR configuration) on the CPU and running base.imgCNN -- and, for
ai2thor_VAR, the modules of base.occupancyCNNMLP up to its Flatten -- at B = 3 under torch autograd in float64 (Policy.double()),
on inputs and weights that are all fp32 numbers, so that the fixture is the reference program's own answer free of fp32 rounding.

The stacks' parameters are overwritten with tests/convstack_cpu.py's convstack_params(kind, 453): seeded Gaussian draws which any
machine reproduces bit for bit from the seed, so no weight is stored (the file keeps check sums of what it used).  The inputs
are tests/convstack_cpu.py's convstack_data: uint8 images, divided by 255 in fp32 as the kernels do, and a seeded d_feat.  The data
seed is the first one from 453 at which torch's fp32 and float64 evaluations have identical ReLU gates and pool choices.

convstack_kuka.npz / convstack_ithor.npz / convstack_occupancy.npz
    image (uint8), d_feat, feat, check.<parameter> (sum, sum of magnitudes); the gradients of sum(feat * d_feat): every bias
    gradient g.d.<parameter> in full, every weight gradient as every 16th output-channel row (.rows16) plus the float64 sums
    over each output channel's (ci, ky, kx) (.rowsum: every row is covered) and over the output channels (.colsum).

usage: make_golden_convstack.py REFERENCE_CHECKOUT
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import convstack_cpu as cc  # noqa: E402
from tests.golden.make_golden_trunk import make_policy  # noqa: E402

B, SEED, ROWS = cc.FIXTURE_B, cc.FIXTURE_SEED, cc.ROWS


def stack_module(kind, bases):
    """The reference's module of a kind: imgCNN, or occupancyCNNMLP's modules up to and including its Flatten."""
    if kind == 2:
        return torch.nn.Sequential(*list(bases[1].occupancyCNNMLP)[:5])
    return bases[kind].imgCNN


def main(reference):
    sys.path.insert(0, reference)
    torch.set_num_threads(4)
    bases = {k: make_policy(k).base for k in (0, 1)}
    for kind in (0, 1, 2):
        mod = stack_module(kind, bases)
        P = cc.convstack_params(kind, SEED)
        sd = mod.state_dict()
        assert [k for k in sd] == cc.param_names(kind), list(sd)
        with torch.no_grad():
            for k, v in P.items():
                assert tuple(sd[k].shape) == v.shape, k
                sd[k].copy_(torch.from_numpy(v))
        mod.double()
        seed = cc.find_seed(kind, B, SEED)
        _P, d, _r64, _r32 = cc.case(kind, B, seed)
        image = torch.from_numpy(cc.as_float_image(d["image"])).double()
        feat = mod(image)
        (feat * torch.from_numpy(d["d_feat"]).double()).sum().backward()
        out = {"image": d["image"], "d_feat": d["d_feat"], "feat": feat.detach().numpy(), "seed": np.int64(SEED), "data_seed": np.int64(seed)}
        params = dict(mod.named_parameters())
        for k in cc.param_names(kind):
            g = params[k].grad
            out["check." + k] = cc.check_values(params[k].detach().numpy())
            if g.dim() == 1:
                out["g.d." + k] = g.numpy()
            else:
                m = g.reshape(g.shape[0], -1)
                out["g.d." + k + ".rows16"] = g[::ROWS].numpy()
                out["g.d." + k + ".rowsum"] = m.sum(1).numpy()
                out["g.d." + k + ".colsum"] = m.sum(0).numpy()
        path = os.path.join(HERE, cc.FIXTURES[kind])
        # everything but the float64 sums is stored as fp32 (half a unit in the last place: 6e-8 of the value)
        keep = lambda k, v: v if (k.endswith(("sum", "seed")) or k.startswith("check.") or v.dtype == np.uint8) else np.asarray(v, dtype=np.float32)   # noqa: E731
        np.savez_compressed(path, **{k: np.ascontiguousarray(keep(k, np.asarray(v))) for k, v in out.items()})
        size = os.path.getsize(path)
        assert size < (1 << 20), (path, size)
        print(path, size, "bytes", "data seed", seed)


if __name__ == "__main__":
    main(sys.argv[1])

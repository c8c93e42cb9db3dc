#!/usr/bin/env python3
"""Golden vectors for the PPO update's MLP trunk, made by IMPORTING the reference's models.ppo.model.Policy for both bases
('arm_VAR', Kuka configuration; 'ai2thor_VAR', iTHOR configuration) on the CPU and running base(obs, hxs, masks) at T = 7,
N = 5 under torch autograd, as PPO.update does on a minibatch -- in float64 (Policy.double()) on inputs, weights and convolution
features that are all fp32 numbers, so that the fixture is the reference program's own answer free of fp32 rounding.

torch.manual_seed(453) before Policy(...).  The trunk's parameters are then overwritten with tests/trunk_cpu.py's trunk_params(kind,
453): seeded Gaussian draws of the initialisation's scale with non-zero biases, which any machine reproduces bit for bit from the
seed, so no weight is stored.  (The constructor's own orthogonal weights are not reproducible that way: nn.init.orthogonal_'s QR
gives weights 1e-4 of their size apart on two machines or thread counts, and the GRU's weight gradient then moves by 2e-5 -- four
times the bound this fixture is compared at.  The file keeps check sums of what it used.)  Seeded observations, a non-zero hxs and
tests/trunk_cpu.py's mask pattern.  A forward hook takes imgCNN's output (and the occupancy convolutions' flattened output): no
image is stored.  The data seed is the first one from 453 at which tests/trunk_cpu.py's fp32 and float64 forwards have identical
ReLU gates (the rule of tests/trunk_cpu.py: the yardstick alone has no flipped gate).

trunk_kuka_t7.npz / trunk_ithor_t7.npz
    feat, motor_in, sound_in, occ (iTHOR), hxs, masks, d_value, d_actor_features, check.<parameter> (sum, sum of magnitudes);
    value, actor_features, h_T; the gradients of sum(value * d_value) + sum(actor_features * d_actor_features):
    g.d_feat, g.d_occ, g.d_hxs and every bias gradient g.d.<parameter> in full, every weight gradient as every 16th row
    (.rows16) plus the float64 sums along both axes (.rowsum: every row is covered, .colsum).
trunk_ithor_t7_gru.npz
    the rows16 of iTHOR's two GRU weight gradients (3072 x 1024 and 3072 x 128), which do not fit the main file's 1 MiB.

usage: make_golden_trunk.py REFERENCE_CHECKOUT
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from tests import trunk_cpu as tc  # noqa: E402

T, N, SEED, ROWS = tc.FIXTURE_T, tc.FIXTURE_N, tc.FIXTURE_SEED, tc.ROWS


class Box:                                   # stand-ins for gym.spaces: Policy reads __class__.__name__ and .shape / .n
    def __init__(self, n):
        self.shape = (n,)


class Discrete:
    def __init__(self, n):
        self.n = n


def make_policy(kind):
    from models.ppo.model import Policy
    torch.manual_seed(SEED)
    if kind == 0:
        cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3, robotStateDim=2)
        return Policy(None, Box(2), base='arm_VAR', config=cfg,
                      base_kwargs={'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 512, 'actionHiddenSize': 128})
    cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3)
    return Policy(None, Discrete(8), base='ai2thor_VAR', config=cfg,
                  base_kwargs={'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 1024, 'actionHiddenSize': 128})


def draw(kind, base, seed):
    """Seeded observations; returns (obs, hxs, masks, d_value, d_actor_features)."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)                  # noqa: E731
    M, H = T * N, tc.hidden(kind)
    obs = {'image': torch.rand(M, 3, 96, 96, generator=g), 'image_feat': rn(M, 3), 'goal_sound_feat': rn(M, 3)}
    if kind == 0:
        obs['robot_pose'] = rn(M, 2)
    else:
        obs['occupancy'] = (torch.rand(M, 1, 9, 9, generator=g) < 0.3).float()
    obs = {k: v.double() for k, v in obs.items()}
    hxs = (0.5 * rn(N, H)).double().requires_grad_()
    masks = tc.trunk_masks(T, N, g).view(M, 1).double()
    return obs, hxs, masks, rn(M, 1).double(), rn(M, 128).double()


def run(kind, base, obs, hxs, masks):
    """The reference's forward with hooks on the convolution stacks' outputs: (value, actor_features, h_T, feat, occ)."""
    taken = {}

    def keep(name):
        def hook(_mod, _inp, out):
            taken[name] = out.detach().float().double().requires_grad_()     # an fp32-representable leaf: what the fixture stores
            return taken[name]
        return hook

    handles = [base.imgCNN.register_forward_hook(keep("feat"))]
    if kind:
        handles.append(base.occupancyCNNMLP[4].register_forward_hook(keep("occ")))     # (Flatten: the first Linear's input)
    value, feats, h_T, _ = base(obs, hxs, masks)
    for h in handles:
        h.remove()
    return value, feats, h_T, taken["feat"], taken.get("occ")


def main(reference):
    sys.path.insert(0, reference)
    torch.set_num_threads(4)
    for kind in (0, 1):
        ac = make_policy(kind)
        base = ac.base
        sd = base.state_dict()
        with torch.no_grad():
            for k, v in tc.trunk_params(kind, SEED).items():
                sd[k].copy_(torch.from_numpy(v))
        ac.double()
        for seed in range(SEED, SEED + 64):
            obs, hxs, masks, d_value, d_actor = draw(kind, base, seed)
            value, feats, h_T, feat, occ = run(kind, base, obs, hxs, masks)
            motor_in = torch.cat([obs['image_feat'], obs['robot_pose']], 1) if kind == 0 else obs['image_feat']
            d = {"feat": feat, "motor_in": motor_in, "sound_in": obs['goal_sound_feat'], "hxs": hxs, "masks": masks}
            if kind:
                d["occ"] = occ
            d = {k: v.detach().numpy().astype(np.float32) for k, v in d.items()}
            P = tc.params_from_base(base, kind)
            with torch.no_grad():
                a64 = tc._forward_only(kind, P, d, torch.float64)
                a32 = tc._forward_only(kind, P, d, torch.float32)
            if tc.same_gates(a64, a32, kind):
                break
        else:
            raise SystemExit("no data seed with identical gates")
        ((value * d_value).sum() + (feats * d_actor).sum()).backward()
        out = dict(d)
        out.update(d_value=d_value.numpy(), d_actor_features=d_actor.numpy(), d_hT=np.zeros((N, tc.hidden(kind)), np.float32),
                   value=value.detach().numpy(), actor_features=feats.detach().numpy(), h_T=h_T.detach().numpy(),
                   seed=np.int64(SEED), data_seed=np.int64(seed))
        out["g.d_feat"], out["g.d_hxs"] = feat.grad.numpy(), hxs.grad.numpy()
        if kind:
            out["g.d_occ"] = occ.grad.numpy()
        extra = {}
        params = dict(base.named_parameters())
        for k in tc.param_names(kind):
            g = params[k].grad
            out["check." + k] = tc.check_values(params[k].detach().numpy())
            if g.dim() == 1:
                out["g.d." + k] = g.numpy()
            else:
                (extra if kind and k.startswith("gru.") else out)["g.d." + k + ".rows16"] = g[::ROWS].numpy()
                out["g.d." + k + ".rowsum"] = g.double().sum(1).numpy()
                out["g.d." + k + ".colsum"] = g.double().sum(0).numpy()
        files = {tc.FIXTURES[kind]: out}
        if extra:
            files[tc.FIXTURES[kind].replace(".npz", "_gru.npz")] = extra
        for name, content in files.items():
            path = os.path.join(HERE, name)
            # everything but the float64 sums is stored as fp32 (half a unit in the last place: 6e-8 of the value)
            keep64 = lambda k: k.endswith(("sum", "seed")) or k.startswith("check.")   # noqa: E731
            np.savez_compressed(path, **{k: np.ascontiguousarray(v if keep64(k) else np.asarray(v, dtype=np.float32))
                                         for k, v in content.items()})
            size = os.path.getsize(path)
            assert size < (1 << 20), (name, size)
            print(path, size, "bytes", "data seed", seed)


if __name__ == "__main__":
    main(sys.argv[1])

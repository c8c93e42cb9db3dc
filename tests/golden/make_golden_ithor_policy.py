#!/usr/bin/env python3
"""Golden vectors for the iTHOR RL actor-critic forward, made by IMPORTING the reference's models.ppo.model.Policy with
base 'ai2thor_VAR' (models/RL/ai2thor_RL_model.py:ai2thorNet_VAR) on CPU, iTHOR configuration (Envs/ai2thor/config.py:
71-85: recurrent, 128 -> 1024 GRU, action hidden 128; img_dim (3,96,96); Discrete(8) actions, RL_env_VAR.py:60).  gym is
not needed: Policy only looks at the action space's class name and .n, so a stand-in class called Discrete is passed.

The 5.5 M weights are not committed: the fixture stores the seed and per-tensor check values, which
var_amd.IthorNetPolicy reproduces with the same constructor order; see tests/test_ithor_policy_host.py.

ithor_policy_b8.npz   inputs of 8 environments (image u8, occupancy u8 in {0, 255}, unit-norm image_feat /
                      goal_sound_feat, rnn_hxs, masks with one episode start), outputs of Policy.act(deterministic=True):
                      value, action (the argmax), action_log_probs, rnn_hxs; base(...) actor features and the logits;
                      a second step fed with the first's rnn_hxs.

usage: make_golden_ithor_policy.py REFERENCE_CHECKOUT
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 453


class Discrete:                              # stand-in for gym.spaces.Discrete: Policy reads __class__.__name__ and .n
    def __init__(self, n):
        self.n = n


def check_values(v):
    f = v.reshape(-1).astype(np.float64)
    return np.concatenate([[f.sum(), np.abs(f).sum()], f[:8]])


def main(reference):
    sys.path.insert(0, reference)
    torch.set_num_threads(4)
    from models.ppo.model import Policy
    cfg = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3)
    torch.manual_seed(SEED)
    ac = Policy(None, Discrete(8), base='ai2thor_VAR', config=cfg,
                base_kwargs={'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 1024, 'actionHiddenSize': 128})
    ac.eval()
    out = {"seed": np.int64(SEED)}
    names = []
    for k, v in ac.state_dict().items():
        names.append(k)
        out["shape." + k] = np.asarray(v.shape, dtype=np.int64)
        out["check." + k] = check_values(v.numpy())
    out["names"] = np.asarray(names)
    rng = np.random.default_rng(37)
    B = 8
    img = rng.integers(0, 256, size=(B, 3, 96, 96), dtype=np.uint8)
    occ = (rng.random((B, 1, 9, 9)) < 0.3).astype(np.uint8) * 255
    unit = lambda a: (a / np.linalg.norm(a, axis=1, keepdims=True)).astype(np.float32)     # noqa: E731
    obs = {
        'image': (torch.from_numpy(img) / 255.).float(),
        'occupancy': (torch.from_numpy(occ) / 255.).float(),
        'image_feat': torch.from_numpy(unit(rng.standard_normal((B, 3)))),
        'goal_sound_feat': torch.from_numpy(unit(rng.standard_normal((B, 3)))),
    }
    hxs = torch.from_numpy(rng.standard_normal((B, 1024)).astype(np.float32) * 0.3)
    masks = torch.ones(B, 1)
    masks[5] = 0.0                                            # env 5 starts a new episode
    out.update(image=img, occupancy=occ, image_feat=obs['image_feat'].numpy(),
               goal_sound_feat=obs['goal_sound_feat'].numpy(), rnn_hxs=hxs.numpy(), masks=masks.numpy())
    with torch.no_grad():
        value, action, logp, hxs1 = ac.act(obs, hxs, masks, deterministic=True)
        _, feats, _, _ = ac.base(obs, hxs, masks)
        logits = ac.dist.linear(feats)
        value2, action2, logp2, hxs2 = ac.act(obs, hxs1, torch.ones(B, 1), deterministic=True)
        _, feats2, _, _ = ac.base(obs, hxs1, torch.ones(B, 1))
    out.update(value=value.numpy(), action=action.numpy(), action_log_probs=logp.numpy(), rnn_hxs_out=hxs1.numpy(),
               actor_features=feats.numpy(), logits=logits.numpy(), value2=value2.numpy(), action2=action2.numpy(),
               action_log_probs2=logp2.numpy(), rnn_hxs_out2=hxs2.numpy(), actor_features2=feats2.numpy())
    np.savez_compressed(os.path.join(HERE, "ithor_policy_b8.npz"), **out)
    print("params", sum(v.numel() for v in ac.state_dict().values()), "keys", len(names))
    print("value", value.numpy().ravel()[:4], "action", action.numpy().ravel(), "logp", logp.numpy().ravel()[:2])


if __name__ == "__main__":
    main(sys.argv[1])

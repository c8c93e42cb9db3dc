#!/usr/bin/env python3
"""Golden vectors for the PPO rollout around the networks, made by IMPORTING the reference's models.ppo.storage.RolloutStorage
and models.ppo.algo.ppo.PPO on the CPU.

rollout_t7.npz   T = 7 steps, N = 5 envs, a dict observation (one member is in config.RLObsIgnore), Discrete actions:
    in.*            what insert() was fed step by step (random masks / bad_masks with both values present) and next_value
    ret.<mode>      returns after compute_returns in the four modes (gae|plain)_(proper|free), vp.<mode> value_preds after it
    adv             the normalised advantages of ppo.py:39-41 from the gae_proper returns (torch fp32)
    perm, mb<i>.*   one recurrent_generator pass with num_mini_batch = 2 under torch.manual_seed(GEN_SEED): the minibatches the
                    reference yields.  N = 5 gives num_envs_per_batch = 2; the reference's loop then indexes perm[5] on its
                    third, short minibatch: mb_count is what it yielded and mb_error the exception's name ('' if none).
    loss<kind>.*    PPO.update (ppo.py:38-104) of one epoch with one minibatch over a stand-in actor-critic whose parameters
                    ARE the values and the head, so that after update() their .grad hold d total / d value, d head (and
                    d logstd); max_grad_norm is huge (the clip multiplies by 1), the Adam step that follows is not recorded.
                    kind 0: DiagGaussian n = 2, kind 1: Categorical n = 4; both with the clipped value loss.

usage: make_golden_rollout.py REFERENCE_CHECKOUT
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
T, N, HID = 7, 5, 4
GEN_SEED = 11
GAMMA, LAMBDA = 0.99, 0.95
CLIP, VCOEF, ECOEF = 0.2, 0.5, 0.01


class Discrete:
    def __init__(self, n):
        self.n = n


class Box:
    def __init__(self, n):
        self.shape = (n,)


def shape(*s):
    return types.SimpleNamespace(shape=s)


def filled(reference_storage, rng, action_space):
    cfg = types.SimpleNamespace(RLObsIgnore=['debug'])
    obs_shape = {'image': shape(2, 3, 3), 'pose': shape(2), 'debug': shape(1)}
    ro = reference_storage(T, N, obs_shape, action_space, HID, cfg)
    f = np.float32
    feed = []
    for t in range(T):
        obs = {'image': rng.normal(size=(N, 2, 3, 3)).astype(f), 'pose': rng.normal(size=(N, 2)).astype(f)}
        if action_space.__class__.__name__ == 'Discrete':
            act = rng.integers(0, action_space.n, size=(N, 1)).astype(np.int64)
        else:
            act = rng.normal(size=(N, action_space.shape[0])).astype(f)
        step = dict(image=obs['image'], pose=obs['pose'], hxs=rng.normal(size=(N, HID)).astype(f), actions=act,
                    logp=(rng.normal(size=(N, 1)) * 0.3 - 1.0).astype(f), value=rng.normal(size=(N, 1)).astype(f),
                    reward=rng.normal(size=(N, 1)).astype(f), masks=(rng.random((N, 1)) < 0.75).astype(f),
                    bad_masks=(rng.random((N, 1)) < 0.75).astype(f))
        feed.append(step)
        tt = {k: torch.from_numpy(v) for k, v in step.items()}
        ro.insert({'image': tt['image'], 'pose': tt['pose']}, tt['hxs'], tt['actions'], tt['logp'], tt['value'], tt['reward'],
                  tt['masks'], tt['bad_masks'])
    assert ro.step == 0
    return ro, feed


def main(reference):
    sys.path.insert(0, reference)
    torch.set_num_threads(1)
    from models.ppo.storage import RolloutStorage
    from models.ppo.algo.ppo import PPO
    from models.ppo.distributions import FixedCategorical, FixedNormal
    rng = np.random.default_rng(71)
    out = {}
    ro, feed = filled(RolloutStorage, rng, Discrete(4))
    for k in feed[0]:
        out["in." + k] = np.stack([s[k] for s in feed])
    masks, bad = ro.masks.numpy(), ro.bad_masks.numpy()
    assert 0 < masks[1:].mean() < 1 and 0 < bad[1:].mean() < 1
    next_value = torch.from_numpy(rng.normal(size=(N, 1)).astype(np.float32))
    out["in.next_value"] = next_value.numpy()
    vp0 = ro.value_preds.clone()
    for name, gae, proper in (("gae_proper", True, True), ("gae_free", True, False), ("plain_proper", False, True),
                              ("plain_free", False, False)):
        ro.value_preds.copy_(vp0)
        ro.returns.zero_()
        ro.compute_returns(next_value, gae, GAMMA, LAMBDA, proper)
        out["ret." + name] = ro.returns.numpy().copy()
        out["vp." + name] = ro.value_preds.numpy().copy()
    ro.value_preds.copy_(vp0)
    ro.compute_returns(next_value, True, GAMMA, LAMBDA, True)
    adv = ro.returns[:-1] - ro.value_preds[:-1]
    adv = (adv - adv.mean()) / (adv.std() + 1e-5)
    out["adv"] = adv.numpy().copy()
    torch.manual_seed(GEN_SEED)
    out["perm"] = torch.randperm(N).numpy()
    torch.manual_seed(GEN_SEED)
    names = ("obs", "recurrent_hidden_states", "actions", "value_preds", "returns", "masks", "action_log_probs", "advantages")
    count, error = 0, ""
    try:
        for sample in ro.recurrent_generator(adv, 2):
            for name, x in zip(names, sample):
                if isinstance(x, dict):
                    for k, v in x.items():
                        out[f"mb{count}.obs.{k}"] = v.numpy().copy()
                else:
                    out[f"mb{count}.{name}"] = x.numpy().copy()
            count += 1
    except IndexError as e:
        error = type(e).__name__
    out["mb_count"], out["mb_error"] = np.int64(count), np.asarray(error)

    # the loss lines, through PPO.update over a stand-in whose parameters are the network outputs
    for kind, space, n in ((0, Box(2), 2), (1, Discrete(4), 4)):
        ro, _ = filled(RolloutStorage, rng, space)
        ro.compute_returns(next_value, True, GAMMA, LAMBDA, True)
        M = T * N

        class StandIn(torch.nn.Module):
            is_recurrent = True

            def __init__(self):
                super().__init__()
                f = np.float32
                self.values = torch.nn.Parameter(torch.from_numpy(rng.normal(size=(M, 1)).astype(f)))
                self.head = torch.nn.Parameter(torch.from_numpy(rng.normal(size=(M, n)).astype(f)))
                if kind == 0:
                    self.logstd = torch.nn.Parameter(torch.from_numpy(rng.uniform(-1, 0, size=(n, 1)).astype(f)))

            def evaluate_actions(self, inputs, rnn_hxs, masks, action):
                self.seen = dict(actions=action, masks=masks)
                if kind == 0:
                    dist = FixedNormal(self.head, (torch.zeros_like(self.head) + self.logstd.t().view(1, -1)).exp())
                else:
                    dist = FixedCategorical(logits=self.head)
                return self.values, dist.log_probs(action), dist.entropy().mean(), rnn_hxs, None

        ac = StandIn()
        samples = []
        gen = ro.recurrent_generator

        def recording(advantages, num_mini_batch):
            for s in gen(advantages, num_mini_batch):
                samples.append(s)
                yield s
        ro.recurrent_generator = recording
        p0 = {k: v.detach().numpy().copy() for k, v in ac.named_parameters()}
        agent = PPO(ac, CLIP, 1, 1, VCOEF, ECOEF, lr=1e-3, eps=1e-5, max_grad_norm=1e30, use_clipped_value_loss=True)
        torch.manual_seed(GEN_SEED + kind)
        vl, al, ent = agent.update(ro)
        assert len(samples) == 1
        _, _, a_b, vp_b, ret_b, _, old_b, adv_b = samples[0]
        pre = f"loss{kind}."
        out[pre + "head"], out[pre + "value"] = p0["head"], p0["values"]
        if kind == 0:
            out[pre + "logstd"] = p0["logstd"].reshape(-1)
            out[pre + "g_logstd"] = ac.logstd.grad.numpy().reshape(-1).copy()
        out[pre + "action"], out[pre + "value_preds"], out[pre + "returns"] = a_b.numpy().copy(), vp_b.numpy().copy(), ret_b.numpy().copy()
        out[pre + "old_logp"], out[pre + "adv"] = old_b.numpy().copy(), adv_b.numpy().copy()
        out[pre + "out"] = np.array([vl, al, ent, vl * VCOEF + al - ent * ECOEF], dtype=np.float64)
        out[pre + "g_head"], out[pre + "g_value"] = ac.head.grad.numpy().copy(), ac.values.grad.numpy().copy()
    path = os.path.join(HERE, "rollout_t7.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; minibatches yielded:", count, "error:", repr(error))


if __name__ == "__main__":
    main(sys.argv[1])

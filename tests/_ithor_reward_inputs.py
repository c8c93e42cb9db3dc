"""Inputs and weights for the iTHOR reward-step tests on which the embeddings are SPREAD.

An untrained encoder maps random images to nearly one point (seed-977 weights, uniform u8 images: the closest two of 8
image_feat rows are 2.2e-4 apart), so a comparison at atol 1e-4 could not see two rows swapped.  The recipe here keeps
the checker's rows at least 2e-3 apart (20x that tolerance): after ithor_seeded(977) every Linear of both heads is
re-drawn from torch.Generator().manual_seed(5) as randn * 3 / sqrt(in_features) (bias randn * 0.5); images are uniform
u8 scaled per row by (i % 8 + 1) / 8; sounds are randn * 6 with column 0 + 18 (drawn as tests/golden/make_golden_ithor.py does) and
row i zeroed from frame 600 - 60 (i % 8) on.  tests/test_ithor_reward_host.py asserts the distances on the CPU."""
import numpy as np
import torch

from oracle.torch_oracle import ithor_seeded      # checker only

MIN_ROW_DISTANCE = 2e-3


def spread_checker(head_seed=5):
    ref = ithor_seeded(977)
    g = torch.Generator().manual_seed(head_seed)
    with torch.no_grad():
        for head in (ref.imgTriplet, ref.soundTriplet):
            for layer in head:
                if isinstance(layer, torch.nn.Linear):
                    layer.weight.copy_(torch.randn(layer.weight.shape, generator=g) * (3.0 / np.sqrt(layer.in_features)))
                    layer.bias.copy_(torch.randn(layer.bias.shape, generator=g) * 0.5)
    return ref.eval()


def spread_inputs(b, seed=21):
    """(images u8 (b,3,96,96), sounds f32 (b,1,600,40)) drawn as tests/golden/make_golden_ithor.py:make_inputs draws them
    (images first, then 2b clips of which the first b are used)."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, size=(b, 3, 96, 96), dtype=np.uint8).astype(np.float64)
    scale = ((np.arange(b) % 8) + 1) / 8.0
    img = np.floor(img * scale[:, None, None, None]).astype(np.uint8)
    snd = rng.standard_normal((2 * b, 1, 600, 40)).astype(np.float32) * 6.0
    snd[:, :, :, 0] += 18.0
    snd = snd[:b].copy()
    for i in range(b):
        snd[i, :, 600 - 60 * (i % 8):] = 0.0
    return img, snd


def spread_images(b, seed=21):
    return spread_inputs(b, seed)[0]


def spread_sounds(b, seed=21):
    return spread_inputs(b, seed)[1]


def checker_image_feat(ref, img_u8):
    with torch.no_grad():
        x = torch.from_numpy(np.ascontiguousarray(img_u8)).float() / 255.0
        return torch.nn.functional.normalize(ref.imgTriplet(ref.imgBranch(x)), p=2, dim=1).numpy()


def checker_goal_feat(ref, snd):
    with torch.no_grad():
        return torch.nn.functional.normalize(ref.soundTriplet(ref.sound_raw(torch.from_numpy(np.ascontiguousarray(snd)))), p=2, dim=1).numpy()


def min_row_distance(rows):
    rows = np.asarray(rows, dtype=np.float64)
    d = np.linalg.norm(rows[:, None, :] - rows[None, :, :], axis=2)
    d[np.arange(len(rows)), np.arange(len(rows))] = np.inf
    return float(d.min())


# ---- the iTHOR actor-critic of the isolation test (constructor arguments of Envs/ai2thor/config.py:71) ----------------
import types  # noqa: E402

POLICY_CFG = types.SimpleNamespace(img_dim=(3, 96, 96), representationDim=3)
POLICY_KW = {'recurrent': True, 'recurrentInputSize': 128, 'recurrentSize': 1024, 'actionHiddenSize': 128}


class Discrete:
    def __init__(self, n):
        self.n = n


def policy_batch(n, seed):
    """(obs dict, rnn_hxs, masks) on the GPU for IthorNetPolicy.act."""
    g = torch.Generator().manual_seed(seed)
    obs = {'image': torch.randint(0, 256, (n, 3, 96, 96), dtype=torch.uint8, generator=g).cuda(),
           'occupancy': ((torch.rand(n, 1, 9, 9, generator=g) < 0.3).to(torch.uint8) * 255).cuda(),
           'image_feat': torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1).cuda(),
           'goal_sound_feat': torch.nn.functional.normalize(torch.randn(n, 3, generator=g), dim=1).cuda()}
    hxs = torch.randn(n, 1024, generator=g).cuda() * 0.3
    masks = (torch.rand(n, 1, generator=g) > 0.2).float().cuda()
    return obs, hxs, masks

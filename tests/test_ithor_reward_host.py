"""Host side of the frozen iTHOR encoder's reward step (var_ithor_reward_*): header, exports, ctypes signatures, the
loud failure without a GPU, and the spread-embedding recipe the GPU tests rely on.  No compute of the library runs here."""
import ctypes
import os
import re
import types

import numpy as np
import pytest
import torch

from tests import _ithor_reward_inputs as rin

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("var_ithor_reward_plan", "var_ithor_reward_pack", "var_ithor_reward_step")


def test_reward_entries_are_declared_and_exported():
    import var_amd
    hdr = open(os.path.join(ROOT, "include", "var_hip.h")).read()
    lib = ctypes.CDLL(var_amd.library_path())
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(var_ctx\*", hdr), f"{name} is not declared in var_hip.h"
        assert hasattr(lib, name), f"{name} is not exported"


def test_reward_entries_have_ctypes_signatures():
    from var_amd._lib import _SIGNATURES, EXPORTED_SYMBOLS
    vp, i, l = ctypes.c_void_p, ctypes.c_int, ctypes.c_long
    assert set(ENTRIES) <= set(EXPORTED_SYMBOLS)
    assert _SIGNATURES["var_ithor_reward_plan"] == (i, [vp, i, i])
    assert _SIGNATURES["var_ithor_reward_pack"] == (i, [vp, vp, vp])
    assert _SIGNATURES["var_ithor_reward_step"] == (i, [vp, vp, vp, vp, i, l, vp, i, vp, vp, vp])


def test_capture_of_a_cpu_ithor_model_fails_loudly():
    import var_amd
    cfg = types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 600, 40), representationDim=3)
    m = var_amd.IthorVARPretextNet(cfg)                       # on the CPU
    with pytest.raises(var_amd.VarHipError):
        var_amd.IntrinsicReward(m).capture(8)


def test_spread_recipe_keeps_the_checkers_rows_apart():
    """The GPU tests compare embeddings at atol 1e-4: the rows they compare must differ by at least 20x that."""
    torch.set_num_threads(8)
    ref = rin.spread_checker()
    img = rin.checker_image_feat(ref, rin.spread_images(8))
    snd = rin.checker_goal_feat(ref, rin.spread_sounds(8))
    di, ds = rin.min_row_distance(img), rin.min_row_distance(snd)
    print(f"min row distance: image_feat {di:.3e}, goal_feat {ds:.3e}")
    assert di >= rin.MIN_ROW_DISTANCE and ds >= rin.MIN_ROW_DISTANCE, (di, ds)
    for seed in (31, 32, 33):                                 # the fresh images of the later steps
        d = rin.min_row_distance(rin.checker_image_feat(ref, rin.spread_images(8, seed)))
        print(f"min row distance: image_feat (seed {seed}) {d:.3e}")
        assert d >= rin.MIN_ROW_DISTANCE, (seed, d)
    assert img.shape == (8, 3) and snd.shape == (8, 3)
    np.testing.assert_allclose(np.linalg.norm(img, axis=1), 1.0, atol=1e-6)

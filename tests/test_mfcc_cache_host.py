"""Host side of the clip cache (VARTrainer(cache_clips=...)): the feature needs the library's var_mfcc_cache_bind /
_unbind; a device context without them -- the oracle context of tests/_oracle_ctx.py -- runs every trainer path exactly as
before, with the new keywords accepted and no extra front-end call."""
import types

import torch

import var_amd
from tests._oracle_ctx import OracleContext


def _cfg():
    return types.SimpleNamespace(img_dim=(3, 84, 84), sound_dim=(1, 100, 40), representationDim=3)


def test_signatures_and_header_carry_the_two_entries():
    from var_amd._lib import EXPORTED_SYMBOLS
    assert "var_mfcc_cache_bind" in EXPORTED_SYMBOLS and "var_mfcc_cache_unbind" in EXPORTED_SYMBOLS
    lib = var_amd.load_library()
    assert lib.var_mfcc_cache_unbind(None) != 0              # no context: an error code, not a crash


def test_oracle_context_runs_uncached_and_unchanged():
    ctx = OracleContext()
    assert not hasattr(ctx.lib, "var_mfcc_cache_bind") and not hasattr(ctx.lib, "var_mfcc_cache_unbind")
    torch.manual_seed(11)
    ma, mb = var_amd.VARPretextNet(_cfg()), var_amd.VARPretextNet(_cfg())
    mb.load_state_dict(ma.state_dict())
    pool = var_amd.SyntheticTripletPool(10, hw=84, seed=3, clips_per_class=2, device="cpu").freeze_pairs()
    B = 4
    table = pool.index_table(B, 2, drop_last=True)[:2].contiguous()
    ta = var_amd.VARTrainer(ma, lr=1e-3, _ctx=ctx)
    assert ta.cache_clips is False and ta._clip_cache(pool.clips, pool.clip_len) is None
    replay, load_table = ta.capture_epoch_steps(pool.images, pool.clips, B, table, clip_len=pool.clip_len)
    got = [float(replay().item()) for _ in range(3)]          # the 3rd replay wraps
    assert [c[0] for c in ctx.lib.calls] == ["loss_grad_pcm", "adam_graph"] * 3       # no cache build, no bind
    ctx_b = OracleContext()
    tb = var_amd.VARTrainer(mb, lr=1e-3, _ctx=ctx_b, cache_clips=False)
    want = []
    for s in range(3):
        r = table[s % 2]
        want.append(float(tb.step_from_dataset(pool.images, r[:B], pool.clips, r[B:3 * B], r[3 * B:],
                                               clip_len=pool.clip_len).item()))
    # (the replayed optimiser reads its learning rate as a float32 from "device" memory, the eager one takes a double)
    assert max(abs(a - b) for a, b in zip(got, want)) < 1e-6, (got, want)
    # (bound of test_trainer_host.py's replayed-vs-eager comparison: Adam steps of lr 1e-3 move an element by up to 1e-3 each,
    #  and where a gradient is tiny the two roundings of the learning rate and of the moments show in m / sqrt(v))
    assert float((ma.flat_parameters() - mb.flat_parameters()).abs().max()) < 2e-5
    assert len(ta._clip_caches) == 0 and len(tb._clip_caches) == 0

"""Duration of the MFCC front-end alone at batch B (default 256 triplets = 512 clips), 20 launches per replayed graph:
without a clip cache, and under var_mfcc_cache_bind with every / half / none of the slots served (a slot is taken out of
the cache by marking its pool row "not cached", so the live work is the same clips' own); then the in-place form of the cached
front-end, the launch the training step makes (var_debug_mfcc_in_place: served and empty slots are not written), on the same
three caches -- where the library has it.
usage: mfcc_time.py [B]"""
import ctypes, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import var_amd
from var_amd._lib import Context, ptr
pool = var_amd.SyntheticTripletPool(2048, hw=84, seed=0, clips_per_class=32).freeze_pairs()
B = int(sys.argv[1]) if len(sys.argv) > 1 else 256
i, c, l = pool.next_batch_indices(B)
ctx = Context.get(0)
n, pcm = c.numel(), pool.clips
out = torch.empty((n, 1, 100, 40), dtype=torch.float32, device="cuda")
feats = var_amd.mfcc(pcm, pool.clip_len).reshape(-1, 100, 40).contiguous()
want = var_amd.mfcc(pcm, l, 100, c)


def launch():
    ctx.check(ctx.lib.var_mfcc(ctx.handle, ctx.stream(), ptr(pcm), ptr(l), ptr(c), n, pcm.stride(0), 100, ptr(out)), "var_mfcc")


def launch_in_place():
    ctx.check(ctx.lib.var_debug_mfcc_in_place(ctx.handle, ctx.stream(), ptr(pcm), ptr(l), ptr(c), n, pcm.stride(0), ptr(out)),
              "var_debug_mfcc_in_place")


def timed(label, clens=None, launch=launch):
    if clens is not None:
        ctx.check(ctx.lib.var_mfcc_cache_bind(ctx.handle, ptr(pcm), pcm.shape[0], pcm.stride(0), 100, ptr(clens), ptr(feats)), "bind")
    launch()
    (g,) = ctx.capture([[launch] * 20])
    ctx.lib.var_mfcc_cache_unbind(ctx.handle)
    for _ in range(3): g()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(10): g()
    e1.record(); torch.cuda.synchronize()
    assert torch.equal(out, want)
    print(f"{label:28s} {e0.elapsed_time(e1) * 1e3 / 200:6.1f} us per launch (back to back in a replayed graph)")


timed("no cache")
rows = torch.arange(pcm.shape[0], device="cuda")
legs = (("cache, every slot served", rows >= 0), ("cache, even rows served", rows % 2 == 0), ("cache, no slot served", rows < 0))
for label, keep in legs:
    timed(label, torch.where(keep, pool.clip_len, torch.full_like(pool.clip_len, -1)).contiguous())
if hasattr(ctx.lib, "var_debug_mfcc_in_place"):
    vp, i = ctypes.c_void_p, ctypes.c_int
    ctx.lib.var_debug_mfcc_in_place.restype, ctx.lib.var_debug_mfcc_in_place.argtypes = i, [vp, vp, vp, vp, vp, i, i, vp]
    # (`out` holds the copying legs' result, so the check inside timed() also says that what the in-place form leaves out is
    # exactly what its readers take from the cache or from nowhere: the live slots it writes are the same bits)
    for label, keep in legs:
        timed("in place: " + label[7:], torch.where(keep, pool.clip_len, torch.full_like(pool.clip_len, -1)).contiguous(),
              launch_in_place)

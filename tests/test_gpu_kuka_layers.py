"""The Kuka contrastive training step (the path bench.py times: img_head2 / img_mid3 / img_chain / img_wgrad345 / img_tail2, snd_*,
heads_*), pinned to float64 LAYER BY LAYER through the C ABI.  One var_arm_encoder_fwd with save_for_bwd = 1 and one
var_arm_encoder_bwd from dense Gaussian cotangents on the three embeddings (every row live; not the triplet hinge); then every
workspace buffer is read back (var_debug_buffer) and each layer is checked alone: the float64 reference of
tests/kuka_layers_cpu.py evaluated on the DEVICE'S OWN input buffers of that layer, against the device's output buffer (or the
slice of the gradient arena).  No error accumulates across layers and no ReLU gate is ambiguous: masks come from the device's own
activations, and every g-buffer holds the gradient wrt its layer's pre-activation (kuka_layers_cpu's docstring: read in the
kernels).  gact1 never exists in memory: conv 1's weight and bias gradients are one composed row from gact2.

Bound per row and output: MARGIN = 4 times layer_distance -- the distance of torch's fp32 CPU kernels from float64 on those same
inputs, relative to the float64 array's largest magnitude (kuka_layers_cpu.ORDER lists the rows measured against an emulation of
the kernel's own accumulation order instead; figures in DESIGN section 2).  Cases A-E also compare the embeddings and the whole
arena end to end with the float64 chain taken at the device's own gates, every differing gate a verified near-tie.

Cases (kuka_layers_cpu.CASES; the smallest shapes that cross each kernel's own limits: kHead2G = kTail2G = 256 persistent
workgroups, kWgG = {512, 256, 64, 32, 32} split-K groups, NU = 4 images per unit of W84_3 / W84_4 / W96_4, NB = 2 bands per image
of W96_2, kSndG = 128, FNC = DNC = 4 clips per sound workgroup, kFusedMaxRows = 1024, fork_ok from B = 33):
  A  h 84, B 1, f32 image: every tile ragged
  B  h 84, B 3, u8 image of 4 channels (batch stride 4 h h), positive sound only: the u8 table path, the channel stride, snd_lo /
     snd_hi with the negative half absent (the zero-filled arena of an absent branch is the last test's)
  C  h 96, B 5: the 96 forms; one full 4-image unit plus one image for W96_4
  D  h 96, B 2 on a plan for at least 5: every B-versus-maxB offset (negative half of sact*, hid_s, emb, gemb, graw, ghid)
  E  h 84, B 37, u8: the side stream taken; W84_3 / W84_4's ragged unit (37 = 9 x 4 + 1)
  F  h 96, B 37, only conv 2-4 weight gradients and the chain's data gradients: W96_2 (74 units on 64 groups) and W96_3 (37 on 32)
  G  h 84, B 65, only the sound rows and conv 2's weight gradient: 130 clips on 128 snd_wgrad groups, the last sound workgroup
     with 2 of 4 clips, 65 units on 64 W84_2 groups
  H  h 84, B 129, only conv 3 / 4 weight gradients and the chain: 33 four-image units (the last with one image) on 32 groups
  I  h 84 and h 96, B 257, only conv 1-2 forward and the gradients of conv 1 and 2: a persistent workgroup of img_head2 /
     img_tail2 walks a second image
then the fused training step (var_arm_loss_grad without feats_out: heads_bwd_fused_kernel at B 5 and 37, the rows + gemm pair
above kFusedMaxRows at B 1025), the forward-only routes, and two bit-for-bit checks."""
import ctypes
import functools
import types

import numpy as np
import pytest
import torch

from tests import kuka_layers_cpu as kc

pytestmark = pytest.mark.gpu

FWD_BUFS = ["sact1", "sact2", "sact3", "sact4", "hid_s", "hid_i", "part", "raw", "emb", "act2", "act3", "act4", "act5", "act1"]
BWD_BUFS = ["gact2", "gact3", "gact4", "gact5", "gsact1", "gsact2", "gsact3", "gsact4", "gemb", "graw", "ghid"]   # (read first:
#             var_debug_buffer("act1") untiles into gact1's block)
HEAD_ROWS = ("fused.heads", "img_head", "snd_head", "img_l2norm", "snd_l2norm")
HEAD_BUFS = ["gact5", "gsact4", "sact4", "hid_s", "hid_i", "part", "raw", "emb", "act5"]


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    # a context of its own: the B = 1025 plan of the fused step would otherwise stay in the process-wide context's grow-only
    # workspace, whose size later modules assume they know
    from var_amd._lib import Context
    OWN["ctx"] = Context(0)
    yield m
    first_run.cache_clear()
    model_for.cache_clear()
    ctx = OWN.pop("ctx")
    torch.cuda.synchronize()
    ctx.lib.var_destroy(ctx.handle)
    ctx.handle = None                                              # (the models' weight images went with it: Weights.__del__ skips them)


OWN = {}


@functools.lru_cache(maxsize=None)
def model_for(var_amd, seed, h):
    m = var_amd.VARPretextNet(types.SimpleNamespace(img_dim=(3, h, h), sound_dim=(1, 100, 40), representationDim=3))
    m.load_state_dict(kc.seeded_params(seed, h))
    return m.to("cuda")


def read_buffers(ctx, B, n, h, image, names):
    """The named workspace buffers cut to the B images and n clips that ran (clips from row B of every (3 maxB) stack)."""
    hs, got = kc.sides(h), {}
    rd = lambda k, shape, offset=0: ctx.debug_buffer(k, int(np.prod(shape)), offset).view(shape)      # noqa: E731
    for k in names:
        l = int(k[-1]) if k[-1].isdigit() else 0
        if k.lstrip("g").startswith("act"):
            if image:
                got[k] = rd(k, (B, kc.ICH[l], hs[l], hs[l]))
        elif k.lstrip("g").startswith("sact"):
            if n:
                got[k] = rd(k, (n, 32, kc.SND_T[l], 1))
        elif k == "hid_i":
            if image:
                got[k] = rd(k, (B, 128))
        elif k == "hid_s":
            if n:
                got[k] = rd(k, (n, 128))
        else:                                                      # rows [images from 0 | clips from B]
            name, w = {"part": ("head_part", 16), "raw": ("emb_raw", 3), "emb": ("emb", 3), "gemb": ("gemb", 3),
                       "graw": ("graw", 4), "ghid": ("ghid", 128)}[k]
            cut = (lambda t: t[:, :3].contiguous()) if k == "graw" else (lambda t: t)
            if image:
                got[k + "_i"] = cut(rd(name, (B, w)))
            if n:
                got[k + "_s"] = cut(rd(name, (n, w), w * B))
    return got


def run_case(var_amd, spec, parts="is", save=1, fused=None, bufs=None):
    """One forward (and backward) of the case through the C ABI ('i' = with the image, 's' = with the sounds): every buffer cut to
    the batch that ran, still on the device, under the names of kuka_layers_cpu; the arena as 'arena'.  fused = (margin,
    inv_count): var_arm_loss_grad instead, its loss as 'loss'."""
    from var_amd._lib import current_stream_handle, ptr
    h, B = spec["h"], spec["B"]
    m = model_for(var_amd, spec["seed"], h)
    ctx = OWN["ctx"]
    ctx.ensure_plan(max(B, spec.get("plan", B)), h)
    flat = m.flat_parameters()
    m.hip_weights(ctx, force=True)
    image, snd, g_i, g_s = kc.make_inputs(spec)
    n = snd.shape[0] if "s" in parts else 0
    img = image.cuda().contiguous() if "i" in parts else None
    pos = snd[:B].cuda().contiguous() if n else None
    neg = snd[B:].cuda().contiguous() if n > B else None
    is_u8, bstride = int(image.dtype == torch.uint8), spec["ch"] * h * h
    s, lib = current_stream_handle(), ctx.lib
    arena = torch.full((len(flat),), float("nan"), device="cuda") if save == 1 else None
    got = {}
    if fused is not None:
        loss = torch.full((1,), float("nan"), device="cuda")
        ctx.check(lib.var_arm_loss_grad(ctx.handle, s, ptr(flat), ptr(img), is_u8, bstride, ptr(pos), ptr(neg), B, h,
                                        ctypes.c_float(fused[0]), ctypes.c_float(fused[1]), ptr(arena), ptr(loss), None), "var_arm_loss_grad")
        got["loss"] = loss
    else:
        feats = [torch.full((B, 3), float("nan"), device="cuda") for _ in range(3)]
        ctx.check(lib.var_arm_encoder_fwd(ctx.handle, s, ptr(flat), ptr(img), is_u8, bstride, ptr(pos), ptr(neg), B, h,
                                          ptr(feats[0]), ptr(feats[1]), ptr(feats[2]), None, None, save), "var_arm_encoder_fwd")
        if save == 1:
            cots = [g_i.cuda() if img is not None else None, g_s[:B].cuda() if n else None, g_s[B:].cuda() if n > B else None]
            ctx.check(lib.var_arm_encoder_bwd(ctx.handle, s, ptr(flat), ptr(cots[0]), ptr(cots[1]), ptr(cots[2]), ptr(arena)),
                      "var_arm_encoder_bwd")
    torch.cuda.synchronize()
    maxB = ctx.debug_buffer_length("emb") // 9
    assert maxB >= max(B, spec.get("plan", B))
    if bufs is None:
        bufs = (BWD_BUFS[:8] if fused is not None else BWD_BUFS if save == 1 else []) + FWD_BUFS
    got.update(read_buffers(ctx, B, n, h, img is not None, bufs), maxB=maxB)
    if arena is not None:
        got["arena"] = arena
    if fused is None:                                              # the embeddings handed to the caller are the workspace's
        for k, f, rows in (("emb_i", feats[0], slice(0, B)), ("emb_s", feats[1], slice(0, B)), ("emb_s", feats[2], slice(B, 2 * B))):
            if k in got and rows.stop <= got[k].shape[0]:
                assert torch.equal(got[k][rows], f), k
    return got


@functools.lru_cache(maxsize=None)
def first_run(var_amd, name):
    return run_case(var_amd, kc.CASES[name])


def part_sum(part, b1):
    """raw = b1 + the four partial sums of the 128 -> 3 layer (rows of 4 x 4 floats, the fourth of each group unused)."""
    return part.view(-1, 4, 4)[:, :, :3].sum(1) + b1


def host_buffers(spec, got, P, parts="is"):
    image, snd, g_i, g_s = kc.make_inputs(spec)
    b = {k: v.cpu() for k, v in got.items() if torch.is_tensor(v) and k != "arena"}
    if "i" in parts:
        b["image"] = image
    if "s" in parts:
        b["snd"] = snd
    if "arena" in got:
        o, arena = 0, got["arena"].cpu()
        for k, p in P.items():
            b["G." + k] = arena[o:o + p.numel()].view(p.shape)
            o += p.numel()
        assert o == arena.numel()
    return b


def check_rows(name, b, P, only=None, fused=None):
    """kuka_layers_cpu.check_layers plus the two rows that tie head_part to emb_raw; prints every row and the worst per kind."""
    log = lambda s: print(f"case {name}: {s}")                      # noqa: E731
    res = kc.check_layers(b, P, only=only, log=log, fused=fused)
    for side, lin in (("i", "imgTriplet"), ("s", "soundTriplet")):
        row = ("img" if side == "i" else "snd") + "_head2.sum"
        if "part_" + side in b and (only is None or only(row)):
            ref, dist = kc.layer_eval(part_sum, [b["part_" + side], P[lin + ".2.bias"]])
            e = kc.rel(b["raw_" + side], ref[0])
            res[row] = ("head partial sum", [(e, dist[0], kc.ratio(e, dist[0]))])
            log(f"{row:16s} err {e:.2e} dist {dist[0]:.2e} ratio {res[row][1][0][2]:.2f}")
    kinds = {}
    for n, (k, r) in res.items():
        w = max(r, key=lambda t: t[2])
        if k not in kinds or (w[2], w[1]) > (kinds[k][1][2], kinds[k][1][1]):
            kinds[k] = (n, w)
    for k, (n, (e, dd, q)) in sorted(kinds.items()):
        print(f"case {name} kind {k:38s} worst {q:.3f} of the bound at {n} (err {e:.2e}, distance {dd:.2e})")
    bad = [(n, r) for n, (_k, r) in res.items() if not all(q <= 1 for _e, _d, q in r)]       # (not "any q > 1": NaN must not pass)
    return res, bad


ROWS = {"A": 50, "B": 50, "C": 50, "D": 50, "E": 50, "F": 6, "G": 25, "H": 5, "I84": 5, "I96": 5}


@pytest.mark.parametrize("name", list(kc.CASES))
def test_every_layer_against_float64(var_amd, name):
    spec = kc.CASES[name]
    got = first_run(var_amd, name)
    P = kc.seeded_params(spec["seed"], spec["h"])
    b = host_buffers(spec, got, P)
    only = (lambda n: n.startswith(spec["only"])) if "only" in spec else None
    res, bad = check_rows(name, b, P, only)
    assert len(res) == ROWS[name], (len(res), sorted(res))
    if "only" not in spec:
        image, snd, g_i, g_s = kc.make_inputs(spec)
        e2e, flips, units = kc.end_to_end(P, image, snd, g_i, g_s, b)
        for k, (err, dist) in e2e.items():
            q = kc.ratio(err, dist)
            print(f"case {name} end to end {k:28s} err {err:.2e} dist {dist:.2e} ratio {q:.2f}")
            if not q <= 1 and not k.startswith("G."):                 # (per tensor: printed; the arena is judged as one array)
                bad.append(("end-to-end " + k, [(err, dist, q)]))
        print(f"case {name} end to end: gates that differ from float64's: {flips} of {units} units")
        bad += [("flip " + k, [(v, tol, n)]) for k, n, v, tol in flips if not v <= tol]
        assert sum(n for _k, n, _v, _t in flips) <= 1 + kc.FLIP_RATE * units, flips
        if not spec["neg"]:                                           # nothing of an absent half is written
            assert got["emb_s"].shape[0] == spec["B"]
    assert not bad, bad


@pytest.mark.parametrize("B", [5, 37, 1025])
def test_fused_training_step_against_float64(var_amd, B):
    """var_arm_loss_grad without feats_out: the loss value, the eight head gradient tensors and gact5 / gsact4 from the device's own
    act5, sact4, hid_* and un-normalised embeddings (the fused step keeps no gemb / graw / ghid); below kFusedMaxRows every other
    row as well, at B 1025 the head rows only."""
    spec = dict(h=84, B=B, u8=True, ch=3, neg=True, seed=40 + B % 7)
    fused = (kc.MARGIN_TRIPLET, 1.0 / B)
    got = run_case(var_amd, spec, fused=fused, bufs=HEAD_BUFS if B > 1024 else None)
    P = kc.seeded_params(spec["seed"], 84)
    b = host_buffers(spec, got, P)
    only = (lambda n: n.startswith(HEAD_ROWS)) if B > 1024 else None
    res, bad = check_rows(f"fused B {B}", b, P, only, fused=fused)
    assert len(res) == (9 if B > 1024 else 41) and len(res["fused.heads"][1]) == 11, (len(res), sorted(res))
    a, p, n = b["emb_i"].double(), b["emb_s"][:B].double(), b["emb_s"][B:].double()
    active = int(((a - p + 1e-6).norm(dim=1) - (a - n + 1e-6).norm(dim=1) + 1 > 0).sum())
    print(f"fused B {B}: loss {float(b['loss']):.6f}, {active} of {B} hinges active")
    assert 0 < active
    assert not bad, bad


ROUTES = {      # name: (B, parts, save_for_bwd): which launches plan_encoder_fwd picks
    "one-launch forward (image only, B 3)": (3, "i", 0),                  # ImgPath::All: img_fwd_all_kernel finishes the embeddings
    "small forward, image only (B 3)": (3, "i", 2),                       # Head1Small + the head's own launch, finished inside it
    "small forward with sound (B 3)": (3, "is", 2),                       # Head1Small; sound heads finished in their launch
    "Head1Mid3 with sound (B 17)": (17, "is", 2),                         # round-2 head + img_mid3; heads_finish_kernel for 34 clips
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_forward_only_routes_against_float64(var_amd, route):
    """The forwards that keep nothing for a backward write the same buffers through other launches (api.hip: plan_encoder_fwd; every
    image route leaves act1..act5 -- act1 as NCHW from the round-2 head, band-tiled from img_fwd_all -- hid_i, the head partials and
    the embeddings; the sound route sact1..sact4, hid_s, partials, embeddings): every forward row of them."""
    B, parts, save = ROUTES[route]
    spec = dict(h=84, B=B, u8=True, ch=3, neg=True, seed=50 + B + save)
    got = run_case(var_amd, spec, parts=parts, save=save)
    P = kc.seeded_params(spec["seed"], 84)
    b = host_buffers(spec, got, P, parts)
    res, bad = check_rows(route, b, P)
    assert sorted(res) == sorted([f"conv{l}.fwd" for l in range(1, 6)] + [f"img_head{l}.fwd" for l in (0, 2)] + ["img_head2.sum", "img_l2norm.fwd"] +
                                 ([f"snd{l}.fwd" for l in range(1, 5)] + [f"snd_head{l}.fwd" for l in (0, 2)] + ["snd_head2.sum", "snd_l2norm.fwd"]
                                  if "s" in parts else [])), sorted(res)
    assert not bad, bad


def same_bits(a, b, keys=None):
    diff = [k for k in (keys or a) if torch.is_tensor(a[k]) and not torch.equal(a[k], b[k])]
    assert not diff, diff


def test_a_second_run_gives_the_same_bits(var_amd):
    first = first_run(var_amd, "C")
    again = run_case(var_amd, kc.CASES["C"])
    assert set(first) == set(again) and len(first) >= 30
    same_bits(first, again)


def test_image_only_and_sound_only_calls_give_the_joint_calls_bits(var_amd):
    joint = first_run(var_amd, "A")
    spans, o = {}, 0
    for k, p in kc.seeded_params(kc.CASES["A"]["seed"], 84).items():
        spans[k] = (o, o + p.numel())
        o += p.numel()
    for parts, mine in (("i", ("imgBranch", "imgTriplet")), ("s", ("soundCNN", "soundTriplet"))):
        half = run_case(var_amd, kc.CASES["A"], parts)
        keys = [k for k in half if k != "arena"]
        assert len(keys) >= 15 and set(keys) <= set(joint)
        same_bits(half, joint, keys)
        for k, (lo, hi) in spans.items():
            if k.startswith(mine):
                assert torch.equal(half["arena"][lo:hi], joint["arena"][lo:hi]), k
                assert float(half["arena"][lo:hi].abs().max()) > 0, k
            else:
                assert float(half["arena"][lo:hi].abs().max()) == 0, k

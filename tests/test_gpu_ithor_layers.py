"""The iTHOR model's fp32 training path (set_precision('fp32'): csrc/ithor.hip over the gather-GEMM of csrc/gg.h), pinned to
float64 LAYER BY LAYER.  One forward under grad and one backward from dense Gaussian cotangents on the embeddings (every row
live; not the triplet hinge); then every workspace buffer is read back (var_debug_buffer's "ithor_" names) and each layer is
checked alone: the float64 reference of tests/ithor_layers_cpu.py evaluated on the DEVICE'S OWN input buffers of that layer,
against the device's output buffer (or the slice of the gradient arena).  No error accumulates across layers and no ReLU gate
is ambiguous: masks come from the device's own activations.

Bound per layer and output: MARGIN = 4 times layer_distance -- the distance of torch's fp32 CPU kernels from float64 on those
same inputs, relative to the float64 array's largest magnitude; routing layers (pools, concatenation) are exact, bound 0.  Four
forward products that run over K >= 1024 on one accumulator missed that bound by the accumulation order alone and are measured
against an emulation of the kernel's order instead (ithor_layers_cpu.ORDER; figures in DESIGN section 8).  The
embeddings and the whole gradient arena are also compared end to end with float64 (ithor_layers_cpu.end_to_end: the chain that
test_ithor_layers_host.py pins to torch.autograd of oracle.torch_oracle.IthorNetCPU, its backward at the device's own gates,
every differing gate a verified near-tie) at MARGIN times the end-to-end fp32 distance.  The pool checks need no tie rule: the
count of windows whose positive maximum is attained twice is required to be 0.

Cases (the model fixes every spatial size; h, B, the inputs present and the image's form are free):
  A  h 84, B 1, all inputs, float image: every product under one 128 x NT tile, conv 6 with M = 9 (its weight gradient's K = 9
     under one chunk), odd maps (21 -> 10: the unfused pool backward; conv 6 on 5 x 5; the stride-2 data gradient with H2 = 3)
  B  h 84, B 3, u8 image of 4 channels (batch stride 4 h h), positive sound only: the u8 loaders of conv 1 forward and weight
     gradient, nclips = B, a ragged last K chunk
  C  h 96, B 5, all, float image: even maps (the fused pool backward), M = 45 and the other ragged tile counts, the wide fold
  D  h 96, B 2, all, on a context planned for 5: every maxB-based offset against every nclips-based stride
  E  h 84, B 33, all, u8: nclips = 66 crosses the 64-column tile of every GRU / head product; conv 6 with M = 297.  Only the
     image layers 5-6 with the head and the sound side from s3 upward are compared (the CPU reference stays small)."""
import functools
import types

import numpy as np
import pytest
import torch

from oracle.torch_oracle import ithor_seeded  # checker only
from tests import ithor_layers_cpu as lc

pytestmark = pytest.mark.gpu

E_ONLY = ("conv5.", "pool5.", "conv6.", "img_head", "img_l2norm", "snd3.bgrad", "gru.", "snd_head", "snd_l2norm")
CASES = {
    "A": dict(h=84, B=1, u8=False, ch=3, neg=True, seed=11),
    "B": dict(h=84, B=3, u8=True, ch=4, neg=False, seed=12),
    "C": dict(h=96, B=5, u8=False, ch=3, neg=True, seed=18),
    "D": dict(h=96, B=2, u8=False, ch=3, neg=True, seed=14, plan=5),
    "E": dict(h=84, B=33, u8=True, ch=3, neg=True, seed=15, only=E_ONLY),
}
IMG_BUFS = [f"a{l}" for l in range(1, 7)] + [f"ga{l}" for l in range(1, 7)] + [f"p{l}" for l in range(2, 6)] + \
           [f"gp{l}" for l in range(2, 6)] + ["hid_i", "ghid_i"]
SND_BUFS = ["s1", "s2", "s3", "gs1", "gs2", "gs3", "gi", "hb", "sraw", "gsraw", "dgi", "dgh", "hid_s1", "ghid_s1", "hid_s2", "ghid_s2"]
E_BUFS = ["p4", "gp4", "a5", "ga5", "p5", "gp5", "a6", "ga6", "hid_i", "ghid_i"] + [k for k in SND_BUFS if k not in ("s1", "s2", "gs1", "gs2")]


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return m


def shapes(B, n, h):
    """Shape of every workspace buffer cut to B images and n clips."""
    hs = lc.sides(h)
    side = lambda l: hs[0] if l <= 2 else hs[l - 2]              # noqa: E731  (output side of conv l = 1..5)
    sh = {"a6": (B, 1152), "hid_i": (B, 128), "s1": (n, 64, 300, 20), "s2": (n, 64, 150, 13), "s3": (n, lc.T, 64, 7),
          "gi": (2, n, lc.T, lc.G3), "dgi": (2, n, lc.T, lc.G3), "dgh": (2, lc.T, n, lc.G3), "hb": (2, lc.T + 1, n, lc.GH),
          "sraw": (n, 1024), "hid_s1": (n, 128), "hid_s2": (n, 64)}
    sh.update({f"a{l}": (B, lc.ICH[l], side(l), side(l)) for l in range(1, 6)})
    sh.update({f"p{l}": (B, lc.ICH[l], hs[l - 1], hs[l - 1]) for l in range(2, 6)})
    grads = {"ga6": "a6", "ghid_i": "hid_i", "gsraw": "sraw", "ghid_s1": "hid_s1", "ghid_s2": "hid_s2"}
    grads.update({f"ga{l}": f"a{l}" for l in range(1, 6)})
    grads.update({f"gp{l}": f"p{l}" for l in range(2, 6)})
    grads.update({f"gs{l}": f"s{l}" for l in range(1, 4)})
    sh.update({g: sh[k] for g, k in grads.items()})
    return sh


def make_inputs(spec):
    h, B = spec["h"], spec["B"]
    rng = np.random.default_rng(100 + spec["seed"])
    img = rng.integers(0, 256, size=(B, spec["ch"], h, h), dtype=np.uint8)
    snd = (rng.standard_normal((2 * B, 1, 600, 40)) * 6.0).astype(np.float32)
    snd[0, :, 350:] = 0.0                                        # one clip silent from frame 350 on
    image = torch.from_numpy(img) if spec["u8"] else (torch.from_numpy(img) / 255.).float()
    cot = torch.from_numpy(rng.standard_normal((3 * B, 3)).astype(np.float32))
    n = 2 * B if spec["neg"] else B
    return image, torch.from_numpy(snd[:n]), cot[:B], cot[B:B + n]


def run_case(var_amd, name, parts="is"):
    """One forward and backward of the case on the device ('i' = with the image, 's' = with the sounds): every buffer cut to the
    batch that ran, still on the device, under the names of ithor_layers_cpu; the arena as 'arena'."""
    from var_amd._lib import Context
    spec = CASES[name]
    h, B = spec["h"], spec["B"]
    ref = ithor_seeded(spec["seed"])
    m = var_amd.IthorVARPretextNet(types.SimpleNamespace(img_dim=(3, h, h), sound_dim=(1, 600, 40), representationDim=3))
    m.load_state_dict(ref.state_dict())
    m = m.to("cuda").set_precision("fp32")
    ctx = Context.get(0)
    if "plan" in spec:
        ctx.check(ctx.lib.var_ithor_plan(ctx.handle, spec["plan"], h), "var_ithor_plan")
    image, snd, g_i, g_s = make_inputs(spec)
    n = snd.shape[0] if "s" in parts else 0
    dev_img = image.cuda() if "i" in parts else None
    pos = snd[:B].cuda() if n else None
    neg = snd[B:].cuda() if n > B else None
    d = m(dev_img, pos, neg)
    outs, cots = [], []
    if dev_img is not None:
        outs.append(d["image_feat"]); cots.append(g_i.cuda())
    if pos is not None:
        outs.append(d["sound_feat_positive"]); cots.append(g_s[:B].cuda())
    if neg is not None:
        outs.append(d["sound_feat_negative"]); cots.append(g_s[B:].cuda())
    torch.autograd.backward(outs, cots)
    torch.cuda.synchronize()
    read = lambda k, count, offset=0: ctx.debug_buffer("ithor_" + k, count, offset)      # noqa: E731
    maxB = ctx.debug_buffer_length("ithor_emb") // 9
    assert maxB >= spec.get("plan", B)
    got = {"arena": torch.cat([p.grad.reshape(-1) for p in m.parameters()]), "maxB": maxB}
    sh = shapes(B, n, h)
    for k in E_BUFS if "only" in spec else IMG_BUFS + SND_BUFS:
        if (k in IMG_BUFS and "i" in parts) or (k in SND_BUFS and n):
            got[k] = read(k, int(np.prod(sh[k]))).view(sh[k])
    for k in ("raw", "graw", "emb"):                              # rows [images from 0 | clips from maxB]
        if "i" in parts:
            got[k + "_i"] = read(k, 3 * B).view(B, 3)
        if n:
            got[k + "_s"] = read(k, 3 * n, 3 * maxB).view(n, 3)
    if "i" in parts:
        torch.testing.assert_close(got["emb_i"], d["image_feat"].detach(), rtol=0, atol=0)
    if n:
        torch.testing.assert_close(got["emb_s"][:B], d["sound_feat_positive"].detach(), rtol=0, atol=0)
    return got


@functools.lru_cache(maxsize=None)
def first_run(var_amd, name):
    return run_case(var_amd, name)


def host_buffers(spec, got, P):
    image, snd, g_i, g_s = make_inputs(spec)
    b = {k: v.cpu() for k, v in got.items() if torch.is_tensor(v) and k != "arena"}
    b.update(image=image, snd=snd, gemb_i=g_i, gemb_s=g_s)
    o, arena = 0, got["arena"].cpu()
    for k, p in P.items():
        b["G." + k] = arena[o:o + p.numel()].view(p.shape)
        o += p.numel()
    assert o == arena.numel()
    return b


@pytest.mark.parametrize("name", list(CASES))
def test_every_layer_against_float64(var_amd, name):
    spec = CASES[name]
    got = first_run(var_amd, name)
    P = {k: v.detach() for k, v in ithor_seeded(spec["seed"]).named_parameters()}
    b = host_buffers(spec, got, P)
    only = (lambda n: n.startswith(spec["only"])) if "only" in spec else None
    res = lc.check_layers(b, P, only=only, log=lambda s: print(f"case {name}: {s}"))
    assert len(res) == (31 if "only" in spec else 62), (len(res), sorted(res))
    bad = [(n, r) for n, (_k, r) in res.items() if not all(q <= 1 for _e, _d, q in r)]       # (not "any q > 1": NaN must not pass)
    kinds = {}
    for n, (k, r) in res.items():
        w = max(r, key=lambda t: t[2])
        if k not in kinds or (w[2], w[1]) > (kinds[k][1][2], kinds[k][1][1]):
            kinds[k] = (n, w)
    for k, (n, (e, dd, q)) in sorted(kinds.items()):
        print(f"case {name} kind {k:14s} worst {q:.3f} of the bound at {n} (err {e:.2e}, fp32 distance {dd:.2e})")
    ties = {l: lc.pool_ties(b[f"a{l}"]) for l in range(2, 6) if f"a{l}" in b}
    print(f"case {name}: pool windows with a repeated positive maximum: {ties}")
    assert not any(ties.values()), ties
    if "only" not in spec:
        image, snd, g_i, g_s = make_inputs(spec)
        e2e, flips, units = lc.end_to_end(P, image, snd, g_i, g_s, b)
        for k, (err, dist) in e2e.items():
            q = lc.ratio(err, dist)
            print(f"case {name} end to end {k:36s} err {err:.2e} dist {dist:.2e} ratio {q:.2f}")
            if not q <= 1 and not k.startswith("G."):                 # (per tensor: printed; the arena is judged as one array)
                bad.append(("end-to-end " + k, [(err, dist, q)]))
        print(f"case {name} end to end: gates / pool routes that differ from float64's: {flips} of {units} units")
        bad += [("flip " + k, [(v, tol, n)]) for k, n, v, tol in flips if not v <= tol]
        assert sum(n for _k, n, _v, _t in flips) <= 1 + lc.FLIP_RATE * units, flips
    assert not bad, bad


def same_bits(a, b, keys=None):
    diff = [k for k in (keys or a) if torch.is_tensor(a[k]) and not torch.equal(a[k], b[k])]
    assert not diff, diff


def test_a_second_run_gives_the_same_bits(var_amd):
    first = first_run(var_amd, "C")
    again = run_case(var_amd, "C")
    assert set(first) == set(again)
    same_bits(first, again)


def test_image_only_and_sound_only_calls_give_the_joint_calls_bits(var_amd):
    joint = first_run(var_amd, "A")
    P = dict(ithor_seeded(CASES["A"]["seed"]).named_parameters())
    spans, o = {}, 0
    for k, p in P.items():
        spans[k] = (o, o + p.numel())
        o += p.numel()
    for parts, mine in (("i", ("imgBranch", "imgTriplet")), ("s", ("rnn", "cnn", "soundTriplet"))):
        half = run_case(var_amd, "A", parts)
        keys = [k for k in half if k != "arena"]
        assert len(keys) >= 19 and set(keys) <= set(joint)
        same_bits(half, joint, keys)
        for k, (lo, hi) in spans.items():
            if k.startswith(mine):
                assert torch.equal(half["arena"][lo:hi], joint["arena"][lo:hi]), k
                assert float(half["arena"][lo:hi].abs().max()) > 0, k
            else:
                assert float(half["arena"][lo:hi].abs().max()) == 0, k

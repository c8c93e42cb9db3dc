"""The iTHOR model's bf16 training path (set_precision('bf16'): csrc/snd_bf16.hip, gru_bf16.hip, img_bf16.hip, dense_bf16.h, the
small_linear_* kernels and the l6_dense_* route of csrc/ithor.hip, csrc/gg.h's bf16 MFMA elsewhere), pinned to float64 LAYER BY
LAYER, in the structure of tests/test_gpu_ithor_layers.py: ithor_seeded weights, one forward under grad and one backward from
dense Gaussian cotangents on the embeddings, every workspace buffer read back (var_debug_buffer's "ithor_" names) and each layer
checked alone by tests/ithor_bf16_layers_cpu.py: the float64 evaluation of the layer ON BF16-ROUNDED PRODUCT OPERANDS, the operands
taken from the device's own fp32 buffers and rounded on the host, against the device's output buffer.  Bound per row and output:
MARGIN = 4 times the distance of torch's fp32 CPU evaluation of the same rounded function from float64; routing rows exact;
ithor_bf16_layers_cpu.ORDER lists the rows measured against an emulation of the kernel's accumulation order instead (DESIGN
section 8).  The layer-wise runs use keep_fp32_activations (var_ithor_set_bf16 mode 2: the fp32 sound maps and, in the sequence
form, the fp32 gate gradients are stored); the production mode 1 is tied to it bit for bit below.  The count of pool windows whose
positive maximum is attained twice is required to be 0.

Cases and the limits each crosses (from the code):
  A  h 96, B 1, all inputs, u8 image, GRU as one launch per pass (gru_bf16_seq_fwd / _bwd).  img_bf16.hip's staged kernels
     (img_bf16_conv takes side 96 / 48 / 24 / 12; ithor.hip:765), layer 5's two-image tile with one half empty; 2 clips, one per
     source, in snd1_bf16_fwd's two-clips-per-CU launch; every head product has rows = 1 | 2 < 64 (dense16::eligible needs M, N
     >= 64, dense_bf16.h:417): small_linear_fwd / _dw / _dx (rows K O <= 80 << 20, ithor.hip:603); the input projection has 146
     rows: the tile kernel of dense_bf16.h on the bf16 copies (resident_a_eligible needs N >= 8 TN = 1024, dense_bf16.h:411)
  B  h 84, B 3, float image, positive sound only.  img_bf16_conv returns 1 for sides 84 / 42 / 21 / 10: layers 2-5 on the
     gather-GEMM with gg.h's bf16 MFMA, odd maps 21 -> 10 (the unfused pool backward, ithor.hip:919) and conv 6 on 5 x 5 below 64
     images (l6_dense_fwd returns 1, ithor.hip:714); one clip source, 3 clips
  C  h 96, B 5, all inputs, u8 image of 4 channels (batch stride 4 h h), context planned for at least 8, GRU as one launch per
     step (set_gru_sequence(False): gru_bf16_step_fwd / _bwd pinned directly).  Every 2 * maxB-based workspace offset of
     snd_bf16 / gru_bf16 / img_bf16 against the nclips-based strides; 730 input-projection rows
  D  h 84, B 33, all inputs, upper layers only.  66 clips: two 64-clip bias slices of the sequence kernel (ncs = 2,
     ithor.hip:1045), the 64-column tiles; rows = 66 >= 64 makes the 1024 -> 128 head eligible: split-K slabs + gg_finish
     (tiles <= 16 and K >= 512, ithor.hip:613); 4818 input-projection rows >= 1024: the resident-A kernel
  E  image only, h 96, B 64: l6_dense_fwd / l6_dense_dgrad at HP = 6 (B >= 64, ithor.hip:714), the image head's 1152 -> 128 on
     split-K + gg_finish from 64 rows.  Only conv 6, its data gradient and the image head
  F  image only, h 84, B 569 = the smallest B with B * 1152 * 128 > 80 << 20 (83886080 / 147456 = 568.9): linear_bwd leaves the
     small_linear kernels for gg() (ithor.hip:637-656; dense_bf16.h's kernel where eligible); l6_dense_* at HP = 5.  Only
     img_head0 and conv 6.  (The sound head's same branch needs 641 clips and is not run: it is the image head's code.)"""
import functools
import types

import numpy as np
import pytest
import torch

from oracle.torch_oracle import ithor_seeded  # checker only
from tests import ithor_bf16_layers_cpu as bl
from tests import ithor_layers_cpu as lc
from tests.test_gpu_ithor_layers import E_BUFS, E_ONLY, IMG_BUFS, SND_BUFS, same_bits, shapes

pytestmark = pytest.mark.gpu

L6_BUFS = ["p5", "gp5", "a6", "ga6", "hid_i", "ghid_i"]
CASES = {
    "A": dict(h=96, B=1, u8=True, ch=3, neg=True, seed=21, rows=62),
    "B": dict(h=84, B=3, u8=False, ch=3, neg=False, seed=22, rows=62),
    "C": dict(h=96, B=5, u8=True, ch=4, neg=True, seed=23, plan=8, steps=True, rows=62),
    "D": dict(h=84, B=33, u8=True, ch=3, neg=True, seed=24, only=E_ONLY, bufs=E_BUFS, rows=31),
    "E": dict(h=96, B=64, u8=True, ch=3, neg=True, seed=25, parts="i", only=("conv6.", "img_head", "img_l2norm"), bufs=L6_BUFS, rows=10),
    "F": dict(h=84, B=569, u8=True, ch=3, neg=True, seed=26, parts="i", only=("conv6.", "img_head0"), bufs=L6_BUFS, rows=6),
}
MODE2_ONLY = ("s1", "s2", "gs1", "gs2")                          # fp32 copies that only keep_fp32_activations stores
MODE2_ONLY_SEQ = ("dgi", "dgh")                                  # ... and, in the sequence form, the fp32 gate gradients


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    torch.set_num_threads(min(16, torch.get_num_threads()))
    return m


def make_inputs(spec, parts="is"):
    h, B = spec["h"], spec["B"]
    rng = np.random.default_rng(300 + spec["seed"])
    img = rng.integers(0, 256, size=(B, spec["ch"], h, h), dtype=np.uint8)
    image = torch.from_numpy(img) if spec["u8"] else (torch.from_numpy(img) / 255.).float()
    cot = torch.from_numpy(rng.standard_normal((3 * B, 3)).astype(np.float32))
    if "s" not in parts:
        return image, None, cot[:B], None
    snd = (rng.standard_normal((2 * B, 1, 600, 40)) * 6.0).astype(np.float32)
    snd[0, :, 350:] = 0.0                                        # one clip silent from frame 350 on
    n = 2 * B if spec["neg"] else B
    return image, torch.from_numpy(snd[:n]), cot[:B], cot[B:B + n]


def run_case(var_amd, name, parts=None, mode=2):
    """One forward and backward of the case on the device in bf16 mode `mode` ('i' = with the image, 's' = with the sounds):
    every buffer cut to the batch that ran, still on the device, under ithor_layers_cpu's names; the arena as 'arena'."""
    from var_amd._lib import Context
    spec = CASES[name]
    parts = parts or spec.get("parts", "is")
    h, B = spec["h"], spec["B"]
    ref = ithor_seeded(spec["seed"])
    m = var_amd.IthorVARPretextNet(types.SimpleNamespace(img_dim=(3, h, h), sound_dim=(1, 600, 40), representationDim=3))
    m.load_state_dict(ref.state_dict())
    m = m.to("cuda").set_precision("bf16", keep_fp32_activations=mode == 2).set_gru_sequence(not spec.get("steps", False))
    ctx = Context.get(0)
    if "plan" in spec:
        ctx.check(ctx.lib.var_ithor_plan(ctx.handle, spec["plan"], h), "var_ithor_plan")
    image, snd, g_i, g_s = make_inputs(spec, parts)
    n = snd.shape[0] if snd is not None else 0
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
    assert ctx.lib.var_ithor_set_bf16(ctx.handle, -1) == mode
    assert m.gru_status() == 0                                   # no hand-off of a persistent GRU launch timed out
    read = lambda k, count, offset=0: ctx.debug_buffer("ithor_" + k, count, offset)      # noqa: E731
    maxB = ctx.debug_buffer_length("ithor_emb") // 9
    assert maxB >= spec.get("plan", B) and ("plan" not in spec or maxB > B)
    got = {"arena": torch.cat([p.grad.reshape(-1) for p in m.parameters()]), "maxB": maxB}
    sh = shapes(B, n, h)
    for k in spec.get("bufs", IMG_BUFS + SND_BUFS):
        if (k in IMG_BUFS and "i" in parts) or (k in SND_BUFS and n):
            got[k] = read(k, int(np.prod(sh[k]))).view(sh[k])
    for k in ("raw", "graw", "emb"):                              # rows [images from 0 | clips from maxB]
        if "i" in parts:
            got[k + "_i"] = read(k, 3 * B).view(B, 3)
        if n:
            got[k + "_s"] = read(k, 3 * n, 3 * maxB).view(n, 3)
    if "i" in parts:
        assert torch.equal(got["emb_i"], d["image_feat"].detach())
    if n:
        assert torch.equal(got["emb_s"][:B], d["sound_feat_positive"].detach())
    return got


@functools.lru_cache(maxsize=None)
def first_run(var_amd, name):
    return run_case(var_amd, name)


def host_buffers(spec, got, P):
    image, snd, g_i, g_s = make_inputs(spec, spec.get("parts", "is"))
    b = {k: v.cpu() for k, v in got.items() if torch.is_tensor(v) and k != "arena"}
    b.update({k: v for k, v in dict(image=image, snd=snd, gemb_i=g_i, gemb_s=g_s).items() if v is not None})
    o, arena = 0, got["arena"].cpu()
    for k, p in P.items():
        b["G." + k] = arena[o:o + p.numel()].view(p.shape)
        o += p.numel()
    assert o == arena.numel()
    return b


@pytest.mark.parametrize("name", list(CASES))
def test_every_bf16_layer_against_float64_on_rounded_operands(var_amd, name):
    spec = CASES[name]
    got = first_run(var_amd, name)
    P = {k: v.detach() for k, v in ithor_seeded(spec["seed"]).named_parameters()}
    b = host_buffers(spec, got, P)
    only = (lambda n: n.startswith(spec["only"])) if "only" in spec else None
    order = bl.order_for(spec["B"], not spec.get("steps", False))       # (the emulated orders of the routes this case takes)
    res = bl.check_layers(b, P, only=only, log=lambda s: print(f"case {name}: {s}"), order=order)
    assert len(res) == spec["rows"], (len(res), sorted(res))
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
    assert not bad, bad


def common_keys(spec, got):
    drop = MODE2_ONLY + (() if spec.get("steps", False) else MODE2_ONLY_SEQ)
    return [k for k in got if k not in drop and torch.is_tensor(got[k])]


@pytest.mark.parametrize("name", ["A", "C"])
def test_the_production_mode_gives_the_test_modes_bits(var_amd, name):
    """Mode 1 (what training runs) against mode 2 (what the layer checks read): the three embeddings, the whole gradient arena
    and every buffer both modes write, bit for bit."""
    keep = first_run(var_amd, name)
    prod = run_case(var_amd, name, mode=1)
    keys = common_keys(CASES[name], keep)
    assert set(prod) == set(keep) and {"arena", "emb_i", "emb_s", "raw_i", "raw_s", "hb", "gi", "gs3", "s3", "ga1"} <= set(keys)
    same_bits(keep, prod, keys)


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


@pytest.mark.parametrize("M,N,K,copies,want", [
    (1536, 146, 448, 1, 1), (1536, 730, 448, 1, 1), (1536, 4818, 448, 1, 2),       # the input projection of cases A, C, D
    (128, 2, 1024, 0, 0), (128, 10, 1024, 0, 0), (128, 66, 1024, 0, 1),            # the sound head's first layer in A, C, D
    (128, 63, 1152, 0, 0), (128, 64, 1152, 0, 1), (128, 569, 1152, 0, 1)])         # the image head's around E's limit and in F
def test_the_dense_routes_the_cases_count_on(var_amd, M, N, K, copies, want):
    """The routes the case list names, by the predicates the step itself asks (dense16::eligible / resident_a_eligible), through
    var_debug_ithor_dense's return convention: 0 = the gather-GEMM fallback (in the step: the small_linear kernels), 1 = the tile
    kernel of dense_bf16.h, 2 = its resident-A kernel (only with both operands as bf16 copies)."""
    from var_amd._lib import Context
    m = var_amd.IthorVARPretextNet(types.SimpleNamespace(img_dim=(3, 96, 96), sound_dim=(1, 600, 40), representationDim=3))
    m = m.to("cuda").set_precision("bf16")
    ctx = Context.get(0)
    m._ensure_plan(ctx, 2)
    g = torch.Generator().manual_seed(M + N + K)
    a, b = torch.randn(M, K, generator=g).cuda(), torch.randn(N, K, generator=g).cuda()      # both k-fast: W (O, K) and X (rows, K)
    out = torch.full((N, M), float("nan"), device="cuda")
    rc = ctx.lib.var_debug_ithor_dense(ctx.handle, None, 1, 1, a.data_ptr(), b.data_ptr(), out.data_ptr(), M, N, K, 1, 2 * copies)
    torch.cuda.synchronize()
    assert rc == want, rc
    assert bool(torch.isfinite(out).all())

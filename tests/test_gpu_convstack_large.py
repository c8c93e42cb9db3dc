"""GPU checks of the convolution stacks (csrc/convstack.hip) at the batch sizes the PPO update runs and up to the documented limit,
in both precisions: both sides of the first batch at which each layer's weight-gradient split cap holds, the update's shapes (200
and 400 images), B = 1024.  The case table comes from tests/convstack_large_cpu.py's restatement of wgrad_split, not from literals.

The big batch stays on the device; the host sees R images' maps, four images' maps and the reduced sums.  Image b of a batch is
distinct[b % R] (R = 8) and d_feat is drawn fresh for every b, so a layer's float64 weight gradient is that of the R distinct
inputs with the copies' g summed in float64 (convstack_large_cpu's docstring).  Per case:
  * batch independence, bit for bit, on the device: every copy's saved maps equal those of image b % R; a second call on the first
    R images alone, and one on the last R (the highest offsets), give the same feat, saved maps and gradient maps as the large
    call.  A row's K order in gg.h (chunks c_lo .. c_hi of its own K, nsplit = 1 in the forward and the data gradient) and in
    img_bf16.hip's per-image tiles does not depend on M, so equality is asserted, and it ties the large batch to B = R, a size
    the float64 pins of tests/test_gpu_convstack.py cover;
  * forward and gated data gradient, layer-locally, at images 0, 1, B - 2 and B - 1 against float64 from the GPU's own
    neighbouring maps, within convstack_bf16_cpu.bounds(kind, 4, rounding=...).  Three fp32 rows with the longest one-accumulator
    K chains (kind 0 act.17 and g.7, kind 1 act.14: K = 2304, 1152, 1152) measured 1.32, 1.10 and 1.003 of that bound on the MI355X
    (1.8e-6, 1.2e-6 and 1.3e-6 of the array's largest magnitude, at B = 147, 400 and 92; the products are per image, so the size
    plays no part) and are held to four distances of the emulation of the kernel's own order instead
    (convstack_large_cpu.chain_bounds: 5.7e-6, 4.8e-6, 3.6e-6), against which they are printed first;
  * weight gradients (with their float64 row and column sums) against the reduced float64 reference from the GPU's own x_l and
    g_l, bias gradients against the float64 sum of the GPU's g_l, within four times the distance of torch's fp32 CPU evaluation
    of the same full-shape product from float64 (convstack_large_cpu.large_bounds: 3 draws up to B = 409, one above);
  * non-triviality.
In bf16 the numeric checks cover the layers the gather-GEMM serves there (convstack_large_cpu.gemm_layers: kind 0 forward and data
gradient of '0', '15', '17', weight gradients of '0', '10', '12', '15', '17'; kind 1 '0', '14' and '0', '8', '11', '14');
img_bf16.hip's own kernels have their wrap cases in tests/test_gpu_convstack_bf16.py.  Kind 2 computes in fp32 under either
name and runs once.  Every case prints what it measured before it asserts."""
import numpy as np
import pytest
import torch

from tests import convstack_bf16_cpu as cb
from tests import convstack_cpu as cc
from tests import convstack_large_cpu as cl

pytestmark = pytest.mark.gpu
SENT = -77.0
R = cl.R_DEFAULT
CASES = [(k, B, layers, p) for k, B, layers in cl.cases() for p in (("fp32",) if k == 2 else ("fp32", "bf16"))]


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy().copy()


def run(var_amd, kind, module, image, d_feat, precision):
    """conv_stack_eval forward + backward over device tensors: 'feat', 'act.<l>', 'g.<l>', 'd.<parameter>' as CUDA tensors."""
    B = image.shape[0]
    gm = torch.full((var_amd.load_library().var_convstack_saved_floats(kind, B),), SENT, device="cuda")
    feat, saved, smap = var_amd.conv_stack_eval(module, image, return_saved=True, precision=precision, grad_maps=gm)
    params = dict(module.named_parameters())
    grads = torch.autograd.grad((feat * d_feat).sum(), [params[k] for k in cc.param_names(kind)])
    res = {"feat": feat.detach()}
    for name, (off, shape) in smap.items():
        n = int(np.prod(shape))
        res["act." + name], res["g." + name] = saved[off:off + n].view(shape), gm[off:off + n].view(shape)
    res.update({"d." + k: g.detach() for k, g in zip(cc.param_names(kind), grads)})
    return res


def per_image(res):
    return [k for k in res if k == "feat" or k.startswith(("act.", "g."))]


@pytest.mark.parametrize("kind,B,layers,precision", CASES)
def test_a_large_batch_is_its_images_and_its_sums_match_float64(var_amd, kind, B, layers, precision):
    rounding = precision == "bf16"
    names, geo = list(cc.layer_names(kind)), cb.geometry(kind)
    for line in cl.describe(kind, B, layers):
        print(line)
    seed = cl.LARGE_SEED + B
    P, d = cc.convstack_params(kind, seed), cl.repeated_data(kind, B, seed, R)
    module = cc.stack_module(kind, P).cuda()
    image, d_feat = dev(d["image"]), dev(d["d_feat"])
    big = run(var_amd, kind, module, image, d_feat, precision)
    assert bool(torch.equal(image, dev(d["image"])))                 # the input is unchanged

    # 1: batch independence, bit for bit, on the device
    idx = torch.arange(B, device="cuda") % R
    for n in names:
        assert bool(torch.equal(big["act." + n], big["act." + n][:R][idx])), f"act.{n}: a copy differs from its image"
        assert not bool((big["g." + n] == SENT).any()), f"g.{n} holds unwritten elements"
    assert bool(torch.equal(big["feat"], big["act." + names[-1]].reshape(B, -1)))
    for lo in (0, B - R):
        sub = run(var_amd, kind, module, image[lo:lo + R].contiguous(), d_feat[lo:lo + R].contiguous(), precision)
        for k in per_image(big):
            assert bool(torch.equal(sub[k], big[k][lo:lo + R])), f"{k} of images {lo}..{lo + R - 1} differs from a call on them alone"
    last = names[-1]
    gate = (big["act." + last] > 0).reshape(B, -1)
    assert bool(torch.equal(big["g." + last].reshape(B, -1), torch.where(gate, d_feat, torch.zeros_like(d_feat))))
    print(f"kind {kind} B {B} {precision}: every copy equals its image; images 0..{R - 1} and {B - R}..{B - 1} equal a call on them alone")

    worst = (0.0, None)

    def hold(k, got, ref, bound):
        nonlocal worst
        err = cb.rel(got, ref)
        assert bound > 0 and np.abs(ref).max() > 0, k
        print(f"    kind {kind} B {B} {precision} {k}: error {err:.3g}, bound {bound:.3g}, fraction {err / bound:.3f}")
        worst = max(worst, (err / bound, (k, err, bound)))

    # 2: forward and gated data gradient, layer-locally, at four images
    images = [0, 1, B - 2, B - 1]
    sub_d = {"image": d["image"][images], "d_feat": d["d_feat"][images]}
    small = {k: host(v[images]) for k, v in big.items() if k.startswith(("act.", "g."))}
    bound4 = cb.bounds(kind, len(images), rounding=rounding)
    conv_layers = cl.gemm_layers(kind, precision, "conv")
    ref = cb.layer_refs(kind, P, sub_d, small, what=("act",), layers=list(conv_layers), rounding=rounding)
    below = [names[names.index(n) - 1] for n in conv_layers if names.index(n) > 0]
    ref.update(cb.layer_refs(kind, P, sub_d, small, what=("g",), layers=below, rounding=rounding))
    assert len(ref) == len(conv_layers) + len(below)
    chain = cl.chain_bounds(kind, len(images)) if precision == "fp32" else {}
    xs4 = cb.layer_inputs(kind, sub_d["image"], small)
    for k in sorted(ref):
        if k in chain:
            # a row of the gather-GEMM's one-accumulator K chain (convstack_large_cpu.CHAIN_ROWS): the GPU against the emulation
            # of that order first, then held to four distances of the emulation, not of torch's blocked sums
            emu = cl.chain_row(kind, k, P, xs4, small)
            print(f"    kind {kind} B {B} {precision} images {images} {k}: error / torch's bound {cb.rel(small[k], ref[k]) / bound4[k]:.3f}; "
                  f"its own order emulated is {cb.rel(emu, ref[k]):.3g} from float64 and {cb.rel(small[k], emu):.3g} from the GPU")
        hold(f"images {images} {k}", small[k], ref[k], chain.get(k, bound4[k]))

    # 3: weight and bias gradients against the reduced float64 reference from the GPU's own x_l and g_l
    checked = [n for n in layers if n in cl.gemm_layers(kind, precision, "wgrad")]
    assert checked
    bounds = cl.large_bounds(kind, B, tuple(checked), rounding)
    first = {k: host(v[:R]) for k, v in big.items() if k.startswith(("act.", "g."))}
    xs = cb.layer_inputs(kind, d["distinct"], first)
    for n in checked:
        l = names.index(n)
        _nm, cin, cout, stride, pad, _pl = geo[l]
        g = big["g." + n]
        gr = g.to(torch.bfloat16).float() if rounding else g
        gsum = torch.stack([gr[i::R].double().sum(0) for i in range(R)]).cpu()
        bsum = g.double().sum((0, 2, 3)).cpu().numpy()
        key = "d." + n + ".weight"
        ref = cl.sums_of(key, cl.reduced_weight_grad(xs[l], gsum, (cout, cin, 3, 3), stride, pad, rounding).numpy())
        got = cl.sums_of(key, host(big[key]))
        for k in ref:
            hold(k, got[k], ref[k], bounds[k])
        hold("d." + n + ".bias", host(big["d." + n + ".bias"]), bsum, bounds["d." + n + ".bias"])

    # 4: non-triviality
    res = dict(first)
    res.update({"d." + k: host(big["d." + k]) for k in cc.param_names(kind)})
    assert cb.nontrivial(kind, res), "a map without positive or without zero units, or a zero gradient array"
    print(f"kind {kind} B {B} {precision}: worst error / bound {worst[0]:.3f} at {worst[1]}")
    assert worst[0] <= 1.0, worst

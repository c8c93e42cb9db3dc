"""The three MFCC kernels (csrc/mfcc.hip in its torchaudio and python_speech_features flavours, csrc/mfcc_any.hip) against the
float64 restatement of oracle/mfcc_np.py at their edges (-m gpu):

  * accuracy in the LOG-MEL domain, with a tolerance that follows the conditioning.  n_mfcc = n_mels = 40 and the DCT is
    orthonormal, so the kernel's log-mel vector is recovered on the host (out @ D^T) and every live (frame, band) is held to
    the first-order bound of oracle.mfcc_np.logmel_bound with K = 4 * K_REF.  K_REF is what a float32 restatement built on
    pocketfft needs on the same table of signals and lengths (measured on the CPU, reproduced by
    tests/test_oracle_mfcc.py::test_k_ref_is_what_the_float32_restatement_needs); the factor 4 is the kernels' allowance for
    a 16 x 16 factorisation with an even/odd real split, float32 table twiddles, the matrix cores' summation order and the
    hardware logarithm.  The python_speech_features flavour overwrites coefficient 0 with the log frame energy, so its
    coefficients 1..39 are held to the same bound pushed through |DCT| and the lifter, coefficient 0 to the energy's own;
  * signals that isolate one stage (silence, constants, Nyquist, single impulses at either end and in the middle, a pure
    tone with quiet bands) at the lengths where the frame-count formulas and the reflect padding change behaviour; every
    sample behind lens[i] and every row no clip names holds 0x7FFF, so one read past the valid range is a large error;
  * placement: the arithmetic of a frame does not depend on where its clip sits, so scattered rows, odd and even row
    strides, tiles that straddle clips and ragged grids must reproduce the single-clip result bit for bit;
  * the C ABI's error paths: a negative code, a message, and an output nobody touched."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import mfcc_np  # noqa: E402

# `python -m oracle.mfcc_np` prints the measured ratios (3.4225... on the constant +32767 clip of 33 samples at 64 / 64 / 16;
# 1.5570... on the constant -32768 clip of 560 samples); rounded up to three digits
K_REF_TA = 3.43
K_REF_PSF = 1.56
K_FACTOR = 4.0

VAR_ERR_ARG = -1
SENTINEL = 12345.5
PAD = mfcc_np.PAD_SAMPLE


@pytest.fixture(scope="module")
def var_amd():
    import var_amd as m
    assert torch.cuda.is_available(), "GPU tests need a GPU"
    return m


@pytest.fixture(scope="module")
def abi(var_amd):
    from var_amd._lib import Context
    return Context.get(0)


def cuda(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def pack_rows(clips, stride, rows=None, at=None):
    """(rows, stride) int16 filled with 0x7FFF, clip i at the start of row at[i] (default: row i)."""
    rows = len(clips) if rows is None else rows
    pcm = np.full((rows, stride), PAD, dtype=np.int16)
    for i, c in enumerate(clips):
        pcm[i if at is None else at[i], :len(c)] = c
    return pcm


def run_abi(abi, entry, pcm, lens, clip_index, out_frames, cfg=None, nclips=None):
    """One call of var_mfcc / var_mfcc_ex / var_mfcc_psf through ctypes on device tensors; returns (nclips, out_frames, 40)."""
    from var_amd._lib import current_stream_handle, ptr
    n = int(lens.numel()) if nclips is None else nclips
    out = torch.full((n, out_frames, 40), SENTINEL, dtype=torch.float32, device="cuda")
    extra = () if cfg is None else tuple(int(v) for v in cfg)
    rc = getattr(abi.lib, entry)(abi.handle, current_stream_handle(), ptr(pcm), ptr(lens), ptr(clip_index), n, int(pcm.shape[1]),
                                 int(out_frames), *extra, ptr(out))
    abi.check(rc, entry)
    torch.cuda.synchronize()
    return out


def bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def ta_case(kind, n, cfg):
    x = mfcc_np.edge_signal(kind, n, seed=n)
    parts = mfcc_np.mfcc_torchaudio_parts(x, *cfg)
    return x, parts["logmel"], mfcc_np.logmel_bound(parts, 1.0)


@functools.lru_cache(maxsize=None)
def psf_case(kind, n):
    x = mfcc_np.edge_signal(kind, n, seed=n)
    parts = mfcc_np.mfcc_psf_parts(x)
    d_en, d_coef = mfcc_np.psf_bounds(parts, 1.0)
    return x, parts["mfcc"], d_en, d_coef


def ta_ratio(out_rows, kind, n, cfg):
    """max over the compared (frame, band) of |recovered log-mel - reference| / bound(K = 1); out_rows may be truncated."""
    _, logmel, bound1 = ta_case(kind, n, cfg)
    t = min(out_rows.shape[0], logmel.shape[0])
    got = mfcc_np.recover_logmel(out_rows[:t])
    assert np.all(np.isfinite(got)), (kind, n, cfg)
    return float(np.max(np.abs(got - logmel[:t]) / bound1[:t]))


def psf_ratio(out_rows, kind, n):
    _, ref, d_en, d_coef = psf_case(kind, n)
    t = min(out_rows.shape[0], ref.shape[0])
    got = out_rows[:t].astype(np.float64)
    assert np.all(np.isfinite(got)), (kind, n)
    return (float(np.max(np.abs(got[:, 0] - ref[:t, 0]) / d_en[:t])),
            float(np.max(np.abs(got[:, 1:] - ref[:t, 1:]) / d_coef[:t])))


def assert_within(ratios, k_ref, what):
    """ratios: {case: ratio}.  Prints the largest (the figure a kernel change moves) before asserting every case."""
    worst = max(ratios, key=ratios.get)
    print(f"{what}: largest |error| / bound(K=1) = {ratios[worst]:.3f} at {worst}; allowed {K_FACTOR} * {k_ref} = {K_FACTOR * k_ref:.2f}")
    bad = {k: round(v, 3) for k, v in ratios.items() if not v <= K_FACTOR * k_ref}
    assert not bad, (what, bad)


# ---- 1 + 2: accuracy on the edge table ------------------------------------------------------------------------------------
TA_CFG = (512, 400, 160)
TA_DEAD = (0, -5)
TA_SHORT = (1, 2, 159, 160, 161, 255, 256)          # below torch.stft's domain: finite output, zero rows behind T


def ta_table(stride):
    cases = [(k, n) for k in mfcc_np.SIGNAL_KINDS for n in mfcc_np.TA_LENGTHS]
    clips = [ta_case(k, n, TA_CFG)[0] for k, n in cases]
    lens = [n for _, n in cases]
    for n in TA_DEAD:                                # "empty" class: the row is all filler and must not be looked at
        cases.append(("dead", n)); clips.append(np.zeros(0, np.int16)); lens.append(n)
    for n in TA_SHORT:
        cases.append(("short", n)); clips.append(mfcc_np.edge_signal("noise_tone", n, seed=n)); lens.append(n)
    return cases, cuda(pack_rows(clips, stride)), cuda(np.array(lens, np.int32))


def check_ta_rows(out, cases, what):
    frames = out.shape[1]
    ratios = {}
    for i, (kind, n) in enumerate(cases):
        T = mfcc_np.ta_frames(n)
        assert np.all(out[i, T:] == 0), (what, kind, n, "rows behind the last live frame")
        if kind == "dead":
            continue
        if kind == "short":
            assert np.all(np.isfinite(out[i])), (what, kind, n)
            continue
        assert frames < T or np.any(out[i, T - 1] != 0), (what, kind, n, "last live frame missing")
        ratios[(kind, n)] = ta_ratio(out[i, :T], kind, n, TA_CFG)
    assert_within(ratios, K_REF_TA, what)


@pytest.mark.parametrize("out_frames", [103, 1, 7, 16, 100])
def test_var_mfcc_edge_table(abi, out_frames):
    """var_mfcc, 9 signals x 12 lengths + empty and too-short clips in one launch; out_frames 103 = T(16000) + 2 compares the
    last live frame and the zero rows behind it, the smaller values truncate.  An odd row stride (per-sample loads only)
    must give the same bits as the even one."""
    cases, pcm, lens = ta_table(16002)
    out = run_abi(abi, "var_mfcc", pcm, lens, None, out_frames)
    check_ta_rows(out.cpu().numpy(), cases, f"var_mfcc out_frames {out_frames}")
    _, pcm_odd, _ = ta_table(16003)
    odd = run_abi(abi, "var_mfcc", pcm_odd, lens, None, out_frames)
    assert torch.equal(bits(odd), bits(out))


def test_var_mfcc_ex_default_configuration_is_var_mfcc(var_amd, abi):
    cases, pcm, lens = ta_table(16002)
    a = run_abi(abi, "var_mfcc", pcm, lens, None, 103)
    b = run_abi(abi, "var_mfcc_ex", pcm, lens, None, 103, cfg=TA_CFG)
    c = var_amd.mfcc(pcm, lens, 103)
    assert torch.equal(bits(a), bits(b)) and torch.equal(bits(a), bits(c[:, 0]))


def test_var_mfcc_lens_beyond_the_row_are_the_row(abi):
    clips = mfcc_np.synth_clips(3, seed=5)
    pcm = cuda(np.concatenate([clips, np.full((1, 16000), PAD, np.int16)]))      # a filler row behind the last clip
    ref = run_abi(abi, "var_mfcc", pcm, cuda(np.array([16000] * 3, np.int32)), None, 103)
    for big in (16001, 16160, 2 ** 31 - 1):
        got = run_abi(abi, "var_mfcc", pcm, cuda(np.array([big, 16000, big], np.int32)), None, 103)
        assert torch.equal(bits(got), bits(ref)), big


@pytest.mark.parametrize("cfg", mfcc_np.EX_CONFIGS, ids=lambda c: "%d-%d-%d" % c)
def test_var_mfcc_ex_edge_table(abi, cfg):
    """var_mfcc_ex over the configurations its header promises; n_fft 64 and 128 reach the filters without a single bin."""
    n_fft, win, hop = cfg
    lengths = mfcc_np.ex_lengths(*cfg)
    cases = [(k, n) for k in mfcc_np.SIGNAL_KINDS for n in lengths]
    clips = [ta_case(k, n, cfg)[0] for k, n in cases]
    stride = max(lengths) + 2 + (max(lengths) & 1)
    frames = 1 + max(lengths) // hop + 2
    cases.append(("dead", 0)); clips.append(np.zeros(0, np.int16))
    lens = cuda(np.array([n for _, n in cases], np.int32))
    out = run_abi(abi, "var_mfcc_ex", cuda(pack_rows(clips, stride)), lens, None, frames, cfg=cfg).cpu().numpy()
    ratios = {}
    for i, (kind, n) in enumerate(cases):
        T = mfcc_np.ta_frames(n, hop)
        assert np.all(out[i, T:] == 0), (cfg, kind, n)
        if kind != "dead":
            ratios[(kind, n)] = ta_ratio(out[i, :T], kind, n, cfg)
    assert_within(ratios, K_REF_TA, f"var_mfcc_ex {cfg}")
    odd = run_abi(abi, "var_mfcc_ex", cuda(pack_rows(clips, stride + 1)), lens, None, frames, cfg=cfg).cpu().numpy()
    assert np.array_equal(odd.view(np.int32), out.view(np.int32))


@pytest.mark.parametrize("out_frames", [601, 1, 7, 16, 100])
def test_var_mfcc_psf_edge_table(var_amd, out_frames):
    """var_mfcc_psf through ops.mfcc_psf: coefficient 0 against the log frame energy, coefficients 1..39 against the
    liftered DCT of the reference's log filterbank energies; 601 = T(96000) + 2."""
    cases = [(k, n) for k in mfcc_np.SIGNAL_KINDS for n in mfcc_np.PSF_LENGTHS]
    clips = [psf_case(k, n)[0] for k, n in cases]
    cases.append(("dead", 0)); clips.append(np.zeros(0, np.int16))
    lens = cuda(np.array([n for _, n in cases], np.int32))
    out = var_amd.mfcc_psf(cuda(pack_rows(clips, 96002)), lens, out_frames=out_frames)[:, 0].cpu().numpy()
    r_en, r_coef = {}, {}
    for i, (kind, n) in enumerate(cases):
        T = mfcc_np.psf_frames(n)
        assert np.all(out[i, T:] == 0), (kind, n)
        if kind == "dead":
            continue
        assert out_frames < T or np.any(out[i, T - 1] != 0), (kind, n, "last live frame missing")
        r_en[(kind, n)], r_coef[(kind, n)] = psf_ratio(out[i, :T], kind, n)
    assert_within(r_en, K_REF_PSF, f"var_mfcc_psf energy, out_frames {out_frames}")
    assert_within(r_coef, K_REF_PSF, f"var_mfcc_psf coefficients 1..39, out_frames {out_frames}")


# ---- 3: placement and tiling ----------------------------------------------------------------------------------------------
ENTRIES = {"var_mfcc": None, "var_mfcc_ex": (1024, 800, 640), "var_mfcc_psf": None}


def entry_clips(entry, count, seed):
    """`count` distinct clips of the entry's flavour with lengths at its edges (one of them empty), and the frames that
    hold the longest of them."""
    if entry == "var_mfcc_psf":
        lens = [96000, 50001, 16000, 400, 300, 95999, 0, 561][:count]
        frames = 600
    else:
        lens = [16000, 12345, 9001, 700, 257 if entry == "var_mfcc" else 513, 15999, 0, 400 if entry == "var_mfcc" else 1921][:count]
        frames = 103
    rng = np.random.default_rng(seed)
    clips = []
    for n in lens:
        t = np.arange(n) / 16000.0
        x = 3000.0 * rng.standard_normal(n) + 8000.0 * np.sin(2 * np.pi * rng.uniform(100.0, 4000.0) * t)
        clips.append(np.round(np.clip(x, -32767, 32767)).astype(np.int16))
    return clips, lens, frames


def alone(abi, entry, clips, lens, frames):
    """Every clip in a launch of its own, in a row of its own length (rounded up to even): (count, frames, 40) on the GPU."""
    outs = []
    for c, n in zip(clips, lens):
        stride = max(2, n + (n & 1))
        outs.append(run_abi(abi, entry, cuda(pack_rows([c], stride)), cuda(np.array([n], np.int32)), None, frames, cfg=ENTRIES[entry]))
    return torch.cat(outs)


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_result_does_not_depend_on_where_a_clip_sits(abi, entry):
    """The same 5 clips alone, as rows scattered through clip_index in a 512-row pool ([pos | neg] layout, permuted, with
    repeats), and with an odd and an even row stride: identical bits."""
    clips, lens, frames = entry_clips(entry, 5, seed=71)
    ref = alone(abi, entry, clips, lens, frames)
    wide = max(lens) + 2
    rng = np.random.default_rng(72)
    rows = rng.choice(512, size=5, replace=False)
    B = 9
    pos, neg = rng.integers(0, 5, size=B), rng.permutation(np.arange(B) % 5)
    which = np.concatenate([pos, neg])
    index = cuda(rows[which].astype(np.int32))
    lens_t = cuda(np.array(lens, np.int32)[which])
    want = bits(ref[torch.from_numpy(which).cuda()])
    strides = (wide, wide + 1) if entry != "var_mfcc_psf" else (wide, wide + 2)
    for stride in strides:
        got = run_abi(abi, entry, cuda(pack_rows(clips, stride, rows=512, at=rows)), lens_t, index, frames, cfg=ENTRIES[entry])
        assert torch.equal(bits(got), want), (entry, stride)
    # rows in order, no index
    got = run_abi(abi, entry, cuda(pack_rows(clips, wide)), cuda(np.array(lens, np.int32)), None, frames, cfg=ENTRIES[entry])
    assert torch.equal(bits(got), bits(ref))


def test_psf_entry_refuses_odd_rows(abi):
    """var_mfcc_psf takes even row strides only (include/var_hip.h): an odd one is refused, nothing is launched."""
    from var_amd._lib import ptr
    pcm, lens = cuda(np.zeros((2, 801), np.int16)), cuda(np.array([800, 800], np.int32))
    out = torch.full((2, 4, 40), SENTINEL, device="cuda")
    rc = abi.lib.var_mfcc_psf(abi.handle, None, ptr(pcm), ptr(lens), None, 2, 801, 4, ptr(out))
    torch.cuda.synchronize()
    assert rc == VAR_ERR_ARG and b"even" in abi.lib.var_last_error(abi.handle) and bool((out == SENTINEL).all())


BATCH_SHAPES = [(1, 1), (3, 7), (17, 16), (512, 100), (33, 101), (9, 600), (70001, 3)]


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_tiles_that_straddle_clips_and_ragged_grids(abi, entry):
    """16-frame tiles straddle clips whenever out_frames % 16 != 0, the persistent grid is ragged, and 70001 x 3 puts flat
    frame numbers near 2.1e5 through the float-reciprocal (clip, frame) mapping with a divisor that is no power of two.
    8 distinct clips repeated through clip_index; every output row must carry the bits of its clip's single-clip result."""
    clips, lens, frames = entry_clips(entry, 8, seed=81)
    ref = alone(abi, entry, clips, lens, 600)                          # (8, 600, 40); truncation is a prefix
    stride = max(lens)
    pcm = cuda(pack_rows(clips, stride))
    lens_np = np.array(lens, np.int32)
    for nclips, out_frames in BATCH_SHAPES:
        which = (np.arange(nclips) * 5 + 3) % 8
        got = run_abi(abi, entry, pcm, cuda(lens_np[which]), cuda(which.astype(np.int32)), out_frames, cfg=ENTRIES[entry])
        want = ref[torch.from_numpy(which).cuda(), :out_frames]
        same = (bits(got) == bits(want)).all(dim=2).all(dim=1)
        assert bool(same.all()), (entry, nclips, out_frames, "first differing clip", int((~same).nonzero()[0]))


# ---- 3 (limit) + 4: error paths through the C ABI ---------------------------------------------------------------------------
def refused(abi, entry, pcm, lens, nclips, stride, out_frames, out, cfg=(), sentinel=None, who=None):
    from var_amd._lib import ptr
    rc = getattr(abi.lib, entry)(abi.handle, None, ptr(pcm), ptr(lens), None, nclips, stride, out_frames, *cfg, ptr(out))
    torch.cuda.synchronize()
    msg = abi.lib.var_last_error(abi.handle)
    assert rc == VAR_ERR_ARG and (who or entry).encode() + b":" in msg, (entry, rc, msg)
    if sentinel is not None:
        assert bool((sentinel == SENTINEL).all()), (entry, "output written by a refused call")
    return msg


def test_too_many_frames_are_refused_before_any_launch(abi):
    """The tile kernel maps flat frame numbers to clips in float32: more than 2^23 frames are refused (tiny buffers: a
    launch would not survive them), and var_mfcc_ex's general kernel refuses what does not fit its int frame count."""
    pcm, lens = cuda(np.zeros((1, 512), np.int16)), cuda(np.array([512], np.int32))
    out = torch.full((4, 40), SENTINEL, device="cuda")
    for entry in ("var_mfcc", "var_mfcc_psf"):
        assert b"too many" in refused(abi, entry, pcm, lens, 4097, 512, 2048, out, sentinel=out)
    assert b"too many" in refused(abi, "var_mfcc_ex", pcm, lens, 4097, 512, 2048, out, cfg=(512, 400, 160), sentinel=out,
                                  who="var_mfcc")                  # (this configuration is var_mfcc's kernel)
    assert b"too many" in refused(abi, "var_mfcc_ex", pcm, lens, 70000, 512, 70000, out, cfg=(1024, 800, 640), sentinel=out)


def test_bad_arguments_are_refused_before_any_launch(abi):
    pcm, lens = cuda(np.zeros((1, 512), np.int16)), cuda(np.array([512], np.int32))
    out = torch.full((4, 40), SENTINEL, device="cuda")
    for cfg in [(32, 32, 8), (1000, 400, 160), (4096, 400, 160), (512, 513, 160), (64, 65, 16), (512, 0, 160), (512, 400, 0),
                (1024, 800, 0), (1024, -1, 640), (1024, 800, -640)]:
        refused(abi, "var_mfcc_ex", pcm, lens, 1, 512, 4, out, cfg=cfg, sentinel=out)
    for entry, cfg in (("var_mfcc", ()), ("var_mfcc_ex", (512, 400, 160)), ("var_mfcc_ex", (1024, 800, 640)), ("var_mfcc_psf", ())):
        refused(abi, entry, None, lens, 1, 512, 4, out, cfg=cfg, sentinel=out)
        refused(abi, entry, pcm, None, 1, 512, 4, out, cfg=cfg, sentinel=out)
        refused(abi, entry, pcm, lens, 1, 512, 4, None, cfg=cfg, sentinel=out)
        for nclips, out_frames, stride in [(0, 4, 512), (-1, 4, 512), (1, 0, 512), (1, -3, 512), (1, 4, 0), (1, 4, -512)]:
            refused(abi, entry, pcm, lens, nclips, stride, out_frames, out, cfg=cfg, sentinel=out)
    # and the entry still works afterwards
    good = run_abi(abi, "var_mfcc", pcm, lens, None, 4)
    assert bool(torch.isfinite(good).all())

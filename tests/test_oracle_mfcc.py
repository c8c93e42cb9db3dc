"""MFCC oracle (oracle/mfcc_np.py).  torchaudio is absent here and the reference holds no
vectors for it, so parity with the dependency is UNPINNED; what can be pinned is the
STFT/power stage against torch.stft (the primitive torchaudio.transforms.Spectrogram calls)
and the textbook properties of the mel/DCT matrices."""
import numpy as np
import torch

from oracle import mfcc_np


def test_power_spectrogram_matches_torch_stft():
    clips = mfcc_np.synth_clips(3, seed=11)
    for c in clips:
        x = torch.from_numpy((c / 32768.0).astype(np.float32))
        st = torch.stft(x, n_fft=512, hop_length=160, win_length=400,
                        window=torch.hamming_window(400), center=True, pad_mode='reflect',
                        normalized=False, onesided=True, return_complex=True)
        ref = st.abs().pow(2.0).numpy().T                     # (T, 257)
        got = mfcc_np.power_spectrogram((c / 32768.0).astype(np.float32))
        assert got.shape == ref.shape == (101, 257)
        assert np.max(np.abs(got - ref)) < 2e-4 * np.max(ref)


def test_window_is_torch_hamming():
    assert np.allclose(mfcc_np.hamming_periodic(400), torch.hamming_window(400).numpy().astype(np.float64), atol=1e-7)


def test_dct_is_orthonormal_and_mel_is_triangular():
    d = mfcc_np.dct_matrix()
    assert np.allclose(d.T @ d, np.eye(40), atol=1e-12)
    fb = mfcc_np.mel_filterbank()
    assert fb.shape == (257, 40) and fb.min() >= 0 and fb.max() <= 1.0
    peaks = fb.argmax(axis=0)
    assert np.all(np.diff(peaks) > 0)                        # HTK mel centres increase


def test_shapes_and_padding():
    c = mfcc_np.synth_clips(1, seed=3)[0]
    f = mfcc_np.mfcc_torchaudio(c)
    assert f.shape == (101, 40)
    assert mfcc_np.process_sound_feat(f).shape == (1, 100, 40)
    short = mfcc_np.mfcc_torchaudio(c[:8000])                # 51 frames -> zero-padded in MFCC domain
    p = mfcc_np.process_sound_feat(short)
    assert p.shape == (1, 100, 40) and np.all(p[0, 51:] == 0) and np.all(p[0, :51] == short)
    # a pure tone concentrates energy in one mel band
    t = np.arange(16000) / 16000.0
    tone = np.round(20000 * np.sin(2 * np.pi * 1000 * t)).astype(np.int16)
    mel = mfcc_np.power_spectrogram((tone / 32768.0).astype(np.float32)) @ mfcc_np.mel_filterbank()
    assert abs(int(mel[50].argmax()) - int(mfcc_np.mel_filterbank()[32].argmax())) <= 1


def test_psf_mfcc_oracle_known_properties():
    """python_speech_features branch (Envs/audioLoader.py:158-161): frame count, energy coefficient, silence floor,
    filterbank shape -- properties of the published algorithm (the package itself is absent: parity unpinned)."""
    from oracle import mfcc_np
    rng = np.random.default_rng(3)
    x = np.round(3000 * rng.standard_normal(16000)).astype(np.int16)
    f = mfcc_np.mfcc_psf(x)
    assert f.shape == (1 + int(np.ceil((16000 - 400) / 160)), 40) and f.dtype == np.float64
    assert mfcc_np.mfcc_psf(x[:300]).shape == (1, 40)
    fb = mfcc_np.psf_filterbanks()
    assert fb.shape == (40, 257) and fb.min() >= 0 and fb.max() <= 1.0
    # coefficient 0 is the log of the frame energy = log(sum |rfft|^2 / 512) of the pre-emphasised, windowed frame
    y = np.append(x[0], x[1:] - 0.97 * x[:-1].astype(np.float64))
    fr = y[160:560] * np.hamming(400)
    e = np.sum(np.abs(np.fft.rfft(fr, 512)) ** 2) / 512
    assert abs(f[1, 0] - np.log(e)) < 1e-9
    # silence: every filterbank energy is replaced by eps before the log
    z = mfcc_np.mfcc_psf(np.zeros(1000, dtype=np.int16))
    assert np.allclose(z[:, 0], np.log(np.finfo(float).eps))
    # scaling the signal by c adds 2 log c to coefficient 0 and sqrt(40)*2 log c to ... only the DC cepstrum: c1.. unchanged
    f2 = mfcc_np.mfcc_psf((x // 2 * 2).astype(np.int16))
    f4 = mfcc_np.mfcc_psf(((x // 2 * 2) // 2).astype(np.int16))
    assert np.allclose(f2[:, 1:], f4[:, 1:], atol=1e-9) and np.allclose(f2[:, 0] - f4[:, 0], 2 * np.log(2.0), atol=1e-9)


# ---- the edge table of tests/test_gpu_mfcc_edges.py: the reference side, checked without a GPU -------------------------
def test_dct_is_orthogonal_so_logmel_can_be_recovered():
    d = mfcc_np.dct_matrix()
    assert d.shape == (40, 40)
    assert np.max(np.abs(d @ d.T - np.eye(40))) < 1e-14 and np.max(np.abs(d.T @ d - np.eye(40))) < 1e-14
    parts = mfcc_np.mfcc_torchaudio_parts(mfcc_np.edge_signal("noise_tone", 12345, seed=1))
    assert np.max(np.abs(mfcc_np.recover_logmel(parts["mfcc"]) - parts["logmel"])) < 1e-12
    assert np.array_equal(parts["mfcc"], mfcc_np.mfcc_torchaudio(mfcc_np.edge_signal("noise_tone", 12345, seed=1)))


def test_small_fft_filterbanks_have_empty_triangles():
    """At n_fft 64 / 128 some of the 40 mel triangles contain no bin: the var_mfcc_ex cases with these sizes are what
    reaches the kernel's empty-filter branch."""
    def empty(n):
        return int(np.sum(np.all(mfcc_np.mel_filterbank(n_fft=n) == 0, axis=0)))
    assert empty(64) == 7 and empty(128) == 1 and empty(256) == 0 and empty(512) == 0


def test_reference_is_defined_on_the_whole_edge_table():
    n_ta = n_psf = 0
    for kind, n, cfg in mfcc_np.k_ref_cases("ta"):
        n_fft, win, hop = cfg
        assert n > n_fft // 2 and win <= n_fft                              # np.pad(mode='reflect') / torch.stft domain
        x = mfcc_np.edge_signal(kind, n, seed=n)
        assert x.dtype == np.int16 and x.shape == (n,)
        parts = mfcc_np.mfcc_torchaudio_parts(x, *cfg)
        assert parts["mfcc"].shape == (1 + n // hop, 40) == (mfcc_np.ta_frames(n, hop), 40)
        for key in ("mfcc", "P", "mel", "logmel", "R"):
            assert np.all(np.isfinite(parts[key])), (kind, n, cfg, key)
        assert np.all(np.sqrt(parts["P"]) <= parts["R"][:, None] * (1 + 1e-12))
        assert np.all(mfcc_np.logmel_bound(parts, 1.0) > 0)
        if kind == "zeros":
            assert np.all(parts["logmel"] == np.log(1e-6))
            assert np.allclose(parts["mfcc"][:, 0], np.sqrt(40.0) * np.log(1e-6), rtol=1e-14)
            assert np.max(np.abs(parts["mfcc"][:, 1:])) < 1e-12
        n_ta += 1
    for kind, n, _ in mfcc_np.k_ref_cases("psf"):
        x = mfcc_np.edge_signal(kind, n, seed=n)
        parts = mfcc_np.mfcc_psf_parts(x)
        T = 1 if n <= 400 else 1 + int(np.ceil((n - 400) / 160))
        assert parts["mfcc"].shape == (T, 40) and T == mfcc_np.psf_frames(n)
        assert np.allclose(parts["mfcc"], mfcc_np.mfcc_psf(x), rtol=1e-12, atol=1e-10)
        for key in ("mfcc", "P", "mel", "logmel", "E", "R"):
            assert np.all(np.isfinite(parts[key])), (kind, n, key)
        d_en, d_coef = mfcc_np.psf_bounds(parts, 1.0)
        assert np.all(d_en > 0) and np.all(d_coef > 0) and d_coef.shape == (T, 39)
        n_psf += 1
    assert n_ta == 9 * (12 + 6 * 4 + 1) and n_psf == 9 * 11
    with np.testing.assert_raises(ValueError):                               # 0 < N <= n_fft // 2: torch.stft refuses
        mfcc_np.mfcc_torchaudio_parts(np.zeros(256, np.int16))


def test_k_ref_is_what_the_float32_restatement_needs():
    """K_REF_* of the GPU module are the measured ratios of `python -m oracle.mfcc_np`, rounded up: the float32
    restatement stays inside them and they are not slack."""
    from tests.test_gpu_mfcc_edges import K_REF_PSF, K_REF_TA
    for flavour, k_ref in (("ta", K_REF_TA), ("psf", K_REF_PSF)):
        got, where = mfcc_np.measure_k_ref(flavour)
        assert 0.9 * k_ref <= got <= k_ref, (flavour, got, k_ref, where)

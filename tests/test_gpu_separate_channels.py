"""Stereo stems from the mono models, end to end on the MI355X: ``Separator.channel_spectra`` / ``separate_channels`` on the DSD
graph (513 bins, overlap 25, mean down-mix) and the iKala graph (513 bins, overlap 20, L + R down-mix), one second of
synthetic stereo audio each.

The network itself is tested elsewhere; here its rectified output ``p`` is taken as the product computed it, so nothing is
ill-conditioned: the estimates are held to the rounding bound of tests/chanmask_ref.py against the float64 reference evaluated at
the product's own ``p`` and magnitudes, the PCM to the tolerance tests/test_gpu_parity.py holds ``dcs_stft_inverse_f32`` to on
its goldens (1e-5).
"""
import os

import numpy as np
import pytest

import deepconvsep_amd as dcs
from deepconvsep_amd.arch import EPS_A
from deepconvsep_amd.separation import to_mono
from deepconvsep_amd.synth import synth_audio, synth_params
from oracle import stft_np

import chanmask_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, HOP, F, TC = 1024, 512, 513, 30
ISTFT_TOL = 1e-5          # test_gpu_parity.py::test_compute_inverse_matches_reference, float32
OVERLAP = {"dsd": 25, "ikala": 20}


def _a3(sep, audio):
    return sep.ctx.to_device(np.stack([audio[:, 0], audio[:, 1], to_mono(audio, sep.arch_name)]), np.float32)


_RUNS = {}


def _run(arch):
    """one separator and one pass per graph, shared by the tests below; the reference is computed once and never modified"""
    if arch not in _RUNS:
        _RUNS[arch] = _make_run(arch)
    return _RUNS[arch]


@pytest.fixture(scope="module", params=["dsd", "ikala"])
def run(request):
    return _run(request.param)


@pytest.fixture(scope="module")
def dsd():
    return _run("dsd")


def _make_run(arch):
    ov = OVERLAP[arch]
    sep = dcs.Separator(arch, synth_params(arch, TC, F, seed=7), 0.3, TC, ov, 32, F, N, HOP, np.hanning)
    audio = 0.5 * synth_audio(44100 + 21, seed=12, channels=2)
    est, mag, ph, p = (sep.ctx.to_host(t) for t in sep.channel_spectra(_a3(sep, audio), want_p=True))
    assert sep.net.arch.eps_mode == EPS_A
    est_ref, mask_ref = chanmask_ref.chanmask_ref(p, mag, ov, "A")
    est_ref.setflags(write=False)
    return dict(arch=arch, ov=ov, sep=sep, audio=audio, est=est, mag=mag, ph=ph, p=p, est_ref=est_ref, mask_ref=mask_ref,
                pcm=sep.separate_channels(audio))


def test_spectra_meet_the_rounding_bound(run):
    est, mag, p, S = run["est"], run["mag"], run["p"], run["sep"].net.S
    T = stft_np.frame_count(run["audio"].shape[0], HOP)
    assert p.shape[0] == S and p.shape[2:] == (TC, F) and p.shape[1] >= 1
    assert est.shape == (2, S, T, F) and mag.shape == run["ph"].shape == (2, T, F) and est.dtype == np.float32
    assert np.isfinite(est).all() and (p >= 0).all()
    lim = chanmask_ref.bound(S, TC, run["ov"], mag.astype(np.float64)[:, None])
    err = np.abs(est - run["est_ref"])
    print("%s: max |est - ref| / bound = %.3g" % (run["arch"], float((err / np.where(lim > 0, lim, 1.0)).max())))
    assert np.all(err <= lim)


def test_pcm_matches_the_oracle_inverse_of_the_reference_spectra(run):
    pcm, L = run["pcm"], run["audio"].shape[0]
    S = run["sep"].net.S
    assert pcm.shape == (L, S, 2) and pcm.dtype == np.float64 and np.isfinite(pcm).all()
    worst = 0.0
    for c in range(2):
        for s in range(S):
            want = stft_np.compute_inverse(run["est_ref"][c, s], run["ph"][c].astype(np.float64), N, HOP, np.hanning)[:L]
            worst = max(worst, float(np.abs(pcm[:, s, c] - want).max()))
    print("%s: max |pcm - oracle| = %.3g (tolerance %g)" % (run["arch"], worst, ISTFT_TOL))
    assert worst < ISTFT_TOL


def test_dual_mono_gives_bitwise_equal_channels(run):
    sep = run["sep"]
    audio = np.repeat(run["audio"][:, :1], 2, axis=1)
    est, mag, ph = (sep.ctx.to_host(t) for t in sep.channel_spectra(_a3(sep, audio)))
    assert np.array_equal(est[0], est[1]) and np.array_equal(mag[0], mag[1]) and np.array_equal(ph[0], ph[1])
    pcm = sep.separate_channels(audio)
    assert np.array_equal(pcm[:, :, 0], pcm[:, :, 1]) and pcm.any()


def _covered(run):
    """samples whole tiles cover, as test_ikala_frame2048_ten_seconds_stereo_matches_oracle counts them"""
    n = run["p"].shape[1]
    return ((n - 1) * (TC - run["ov"]) + TC - 4) * HOP - N


def test_stems_of_a_channel_add_up_to_that_channel(run):
    """Convention-A masks partition the mixture and the cross-fade weights of a frame sum to one: each channel's stems add up
    to that channel wherever whole tiles cover the signal (margin of test_ikala_frame2048_ten_seconds_stereo_matches_oracle)."""
    pcm, audio = run["pcm"], run["audio"]
    hi = _covered(run)
    assert hi > 4 * N
    err = np.abs(pcm.sum(axis=1)[N:hi] - audio[N:hi]).max()
    print("%s: max |sum of stems - channel| = %.3g" % (run["arch"], float(err)))
    assert err < 2e-5


def test_cancelling_down_mix(dsd):
    """R = -L: the mean down-mix is exactly zero, so ``sep / x`` would be 0 / 0; the masks exist on their own.  The stems are
    finite, those of R are the negated stems of L, and -- the masks of convention A sum to one whatever the network puts out on
    all-zero tiles -- they still add up to each channel.  Negation: both channels have the same magnitudes, hence bitwise equal
    estimates, and phases pi apart; each PCM is within ISTFT_TOL of the exact inverse, so their sum is within twice that."""
    run = dsd
    sep = run["sep"]
    left = run["audio"][:, 0]
    audio = np.stack([left, -left], axis=1)
    assert not to_mono(audio, "dsd").any()
    est, mag, ph = (sep.ctx.to_host(t) for t in sep.channel_spectra(_a3(sep, audio)))
    assert np.isfinite(est).all() and np.array_equal(est[0], est[1])
    pcm = sep.separate_channels(audio)
    assert np.isfinite(pcm).all() and pcm.any()
    assert np.abs(pcm[:, :, 0] + pcm[:, :, 1]).max() < 2 * ISTFT_TOL
    hi = _covered(run)
    err = np.abs(pcm.sum(axis=1)[N:hi] - audio[N:hi]).max()
    print("cancelling down-mix: max |sum of stems - channel| = %.3g" % float(err))
    assert err < 2e-5


def test_mwf_chain_is_the_composition_of_its_stages(run):
    sep, audio = run["sep"], run["audio"]
    L, S = audio.shape[0], sep.net.S
    ctx = sep.ctx
    est, mag, ph = sep.channel_spectra(_a3(sep, audio))
    # mwf_iters = 0: one inverse per channel with that channel's phase
    for c in range(2):
        pcm = ctx.to_host(sep.plan.inverse(est[c], ph[c], n_out=L, pre_div=1.0))
        assert np.array_equal(pcm.T.astype(np.float64), run["pcm"][:, :, c]), c
    assert np.array_equal(sep.separate_channels(audio, mwf_iters=0), run["pcm"])
    got = sep.separate_channels(audio, mwf_iters=2)
    assert got.shape == run["pcm"].shape and np.isfinite(got).all() and not np.array_equal(got, run["pcm"])
    om, op = ctx.mwf(mag, ph, est, 2, pre_div=1.0)
    for c in range(2):
        for j in range(S):
            pcm = ctx.to_host(sep.plan.inverse(om[c, j], op[c, j], n_out=L))
            assert np.array_equal(pcm.astype(np.float64), got[:, j, c]), (c, j)


def test_another_sample_rate_goes_through_the_resampler(dsd):
    sep = dsd["sep"]
    audio = 0.5 * synth_audio(48000 + 5, seed=3, channels=2)
    got = sep.separate_channels(audio, sample_rate=48000)
    assert got.shape == (audio.shape[0], sep.net.S, 2) and np.isfinite(got).all() and got.any()


def test_multi_channel_graphs_and_bad_input_are_refused(dsd):
    run = dsd
    ild = dcs.Separator("dsd_ild", synth_params("dsd_ild", TC, F, seed=7), 0.3, TC, 25, 32, F, N, HOP, np.hanning, tiler="library")
    with pytest.raises(ValueError):
        ild.separate_channels(run["audio"])
    with pytest.raises(ValueError):
        ild.channel_spectra(_a3(run["sep"], run["audio"]))
    with pytest.raises(ValueError):
        run["sep"].separate_channels(run["audio"][:, 0])
    with pytest.raises(IndexError):                       # too short for one tile: what separate_stepwise raises
        run["sep"].separate_channels(run["audio"][:5000])


def test_script_writes_two_channel_stems(dsd, tmp_path):
    """separate_dsd.py --stereo --mwf 1: the usual file names, two-channel files, the int16 truncation of
    ``separate_channels(audio, mwf_iters=1)``; a mono file is separated as without the switch."""
    run = dsd
    import importlib.util
    import scipy.io.wavfile
    from deepconvsep_amd.separation import read_wav, save_model, write_wav
    spec = importlib.util.spec_from_file_location("separate_dsd", os.path.join(ROOT, "examples", "dsd100", "separate_dsd.py"))
    script = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(script)
    model, wav, mono, out = str(tmp_path / "m.pkl"), str(tmp_path / "mix.wav"), str(tmp_path / "mono.wav"), str(tmp_path)
    save_model(model, synth_params("dsd", TC, F, seed=7))
    write_wav(wav, run["audio"], 44100)
    script.main(["-i", wav, "-o", out, "-m", model, "--stereo", "--mwf", "1"])
    _, audio = read_wav(wav)
    want = run["sep"].separate_channels(audio, mwf_iters=1)
    for i, name in enumerate(("vocals", "bass", "drums", "other")):
        rate, got = scipy.io.wavfile.read(os.path.join(out, name + ".wav"))
        assert rate == 44100 and got.dtype == np.int16 and got.shape == (len(audio), 2)
        assert np.array_equal(got, (want[:, i, :] * 32767).astype(np.int16)), name
    write_wav(mono, run["audio"][:, 0], 44100)
    script.main(["-i", mono, "-o", out, "-m", model, "--stereo"])
    _, a1 = read_wav(mono)
    plain = run["sep"].separate(a1)
    for i, name in enumerate(("vocals", "bass", "drums", "other")):
        rate, got = scipy.io.wavfile.read(os.path.join(out, name + ".wav"))
        assert got.shape == (len(a1),) and np.array_equal(got, (plain[i] * 32767).astype(np.int16)), name

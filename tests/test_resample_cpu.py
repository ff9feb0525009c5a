"""Sample-rate conversion without a GPU: the host design against the float64 restatement tests/resample_ref.py, the
restatement against scipy and against the filter's published figures, the C ABI's symbols and the command lines."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

import resample_ref as ref
from deepconvsep_amd import _lib
from deepconvsep_amd.resample import design, out_length, ratio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("fi,fo", ref.PAIRS)
def test_design_is_the_reference_filter(fi, fo):
    up, down, taps, H = design(fi, fo)
    assert (up, down) == ref.RATIOS[(fi, fo)] == ratio(fi, fo)
    want, want_H = ref.taps(up, down)
    assert H == want_H and taps.dtype == np.float64 and taps.shape == (2 * H + 1,)
    assert np.array_equal(taps, want)
    assert np.array_equal(taps, taps[::-1])                       # h[t] == h[-t]
    assert abs(taps.sum() / up - 1.0) < 1e-6                      # DC gain 1 - 2.5e-7


def test_design_options_and_table_lengths():
    assert design(48000, 44100)[2].size == 10781 and design(44100, 48000)[2].size == 10781
    for fi in (32000, 16000, 8000):
        assert design(fi, 44100)[2].size == 29711
    up, down, taps, H = design(2, 3, zero_crossings=2)            # 3/2 with two crossings: small enough to read
    want, want_H = ref.taps(3, 2, zero_crossings=2)
    assert (up, down, H) == (3, 2, want_H) == (3, 2, 7) and np.array_equal(taps, want)
    assert taps[H] == pytest.approx(0.95) and taps[0] == 0.0      # centre up / R = rolloff; t = -7 lies past Z R = 6.32
    with pytest.raises(ValueError):
        ratio(0, 44100)
    with pytest.raises(ValueError):
        design(48000, 44100, rolloff=0.0)


@pytest.mark.parametrize("fi,fo", ref.PAIRS)
def test_out_length(fi, fo):
    up, down = ratio(fi, fo)
    lib = _lib.load()
    Ls = [0, 1, 2, 3000, 480000]
    for L in (down, 7 * down):                                    # L up is a multiple of down: one either side too
        Ls += [L - 1, L, L + 1]
    for L in Ls:
        want = int(np.ceil(L * up / down)) if L * up % down else L * up // down
        assert out_length(L, up, down) == want == ref.length(L, up, down), L
        assert lib.dcs_resample_length(L, up, down) == want, L
    assert out_length(down, up, down) == up and out_length(down + 1, up, down) == up + -(-up // down)
    assert out_length(out_length(3001, up, down), down, up) >= 3001          # there and back is never shorter
    assert lib.dcs_resample_length(-1, up, down) == -1 and lib.dcs_resample_length(1, 0, down) == -1
    assert lib.dcs_resample_length(1, up, 0) == -1 and lib.dcs_resample_length(2 ** 62, 147, 160) == -1
    with pytest.raises(ValueError):
        out_length(-1, up, down)


@pytest.mark.parametrize("fi,fo", ref.PAIRS)
def test_reference_is_scipys_resample_poly(fi, fo):
    """Both are float64 sums of fewer than 150 terms of magnitude below 1 in different orders: 2.7e-15 apart where this was
    written, 1e-12 asked."""
    signal = pytest.importorskip("scipy.signal")
    up, down = ref.lowest_terms(fi, fo)
    h, H = ref.taps(up, down)
    x = np.random.RandomState(fi % 977).uniform(-1.0, 1.0, 3000)
    got = ref.resample(x, up, down, h, H)
    want = signal.resample_poly(x, up, down, window=h / up)
    assert got.shape == want.shape == (ref.length(3000, up, down),)
    err = float(np.max(np.abs(got - want)))
    print("%d -> %d: max |reference - resample_poly| = %.3g" % (fi, fo, err))
    assert err <= 1e-12


@pytest.mark.parametrize("fi,fo", [(48000, 44100), (44100, 48000)])
def test_filter_figures(fi, fo):
    """The definition's figures on the reference (they pin the definition, not the kernel): a tone at 0.40 min(fi, fo) comes
    through at >= 120 dB SNR (122 dB measured), one 6 % above the new Nyquist at <= -95 dB (-97.6 dB measured)."""
    up, down = ref.lowest_terms(fi, fo)
    h, H = ref.taps(up, down)
    n = np.arange(3000)
    f_pass = 0.40 * min(fi, fo)
    y = ref.resample(np.sin(2 * np.pi * f_pass * n / fi), up, down, h, H)
    m = np.arange(y.size)
    lo, hi = int(0.2 * y.size), int(0.8 * y.size)
    want = np.sin(2 * np.pi * f_pass * m / fo)
    snr = 10 * np.log10(np.sum(want[lo:hi] ** 2) / np.sum((y - want)[lo:hi] ** 2))
    print("%d -> %d: tone at %.0f Hz, SNR %.1f dB" % (fi, fo, f_pass, snr))
    assert snr >= 120.0
    if fo < fi:
        f_stop = 1.06 * fo / 2
        y = ref.resample(np.sin(2 * np.pi * f_stop * n / fi), up, down, h, H)
        level = 20 * np.log10(np.sqrt(np.mean(y[int(0.2 * y.size):int(0.8 * y.size)] ** 2)) / np.sqrt(0.5))
        print("%d -> %d: tone at %.0f Hz (1.06 x the new Nyquist) comes out at %.1f dB" % (fi, fo, f_stop, level))
        assert level <= -95.0


def test_symbols_and_argument_checks():
    names = ("dcs_resample_length", "dcs_resample_plan", "dcs_resample_plan_destroy", "dcs_resample_f32")
    assert set(names) <= set(_lib.header_symbols())
    lib = _lib.load()
    for name in names:
        assert hasattr(lib, name), name
    # the factor checks come before anything touches the context: no device is needed to see them
    taps = np.ones(1)
    h = ctypes.c_void_p()
    for up, down, half in ((0, 1, 0), (1, 0, 0), (-3, 2, 0), (1, 1, -1)):
        rc = lib.dcs_resample_plan(None, up, down, taps.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), half, ctypes.byref(h))
        assert rc == _lib.DCS_EINVAL and not h.value, (up, down, half)
    assert lib.dcs_resample_plan_destroy(None) == _lib.DCS_OK
    assert lib.dcs_resample_f32(None, None, 4, 1, 4, None, 4) == _lib.DCS_EINVAL


def test_package_exports():
    import deepconvsep_amd as dcs
    assert callable(dcs.resample) and isinstance(dcs.Resampler, type)
    assert "resample" in dcs.__all__ and "Resampler" in dcs.__all__


SCRIPTS = ["examples/dsd100/separate_dsd.py", "examples/ikala/separate_ikala.py", "examples/hiphopss/separate_hhds.py",
           "examples/bach10/separate_bach10.py", "examples/bach10_scoreinformed/separate_bach10.py",
           "examples/dsd100_2ch_ILD/separate_dsd_ild.py", "examples/separate_batch.py"]


@pytest.mark.parametrize("script", SCRIPTS)
def test_command_lines_take_resample(script):
    """``--resample -h`` parses (usage or help, exit 0; an unknown option is exit 2 in all of them) and the text names the option."""
    run = subprocess.run([sys.executable, os.path.join(ROOT, script), "--resample", "-h"], stdout=subprocess.PIPE,
                         stderr=subprocess.STDOUT, universal_newlines=True, timeout=120)
    assert run.returncode == 0, run.stdout
    assert "--resample" in run.stdout

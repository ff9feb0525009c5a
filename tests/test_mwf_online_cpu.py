"""Properties of the online multichannel Wiener filter's NumPy oracle (tests/mwf_online_ref.py), so that it cannot drift,
and the library's side of the contract that needs no GPU: the header declares the ``dcs_mwf_online_*`` entry points,
``_lib.py`` binds them and ``libdcs.so`` exports them."""
import ctypes

import numpy as np
import pytest

from deepconvsep_amd import _lib
from mwf_online_ref import gpu_cases, mwf_online_closed, mwf_online_em, run_key, sdr
from mwf_ref import make_case, mixture

SYMBOLS = ("dcs_mwf_online_create", "dcs_mwf_online_destroy", "dcs_mwf_online_reset", "dcs_mwf_online_bytes",
           "dcs_mwf_online_frames", "dcs_mwf_online_push_f32")


@pytest.fixture(scope="module")
def panned():
    return make_case(3, 37, 70, seed=1)


def test_zero_iterations_are_the_identity(panned):
    mag, phase, A, _ = panned
    y, state = mwf_online_em(mag, phase, A, 0)
    assert state is None
    assert np.array_equal(np.abs(y).astype(np.float32), A)
    unit = np.exp(1j * phase.astype(np.float64))
    assert np.allclose(y, A * unit[:, None], rtol=0, atol=1e-12 * A.max())
    assert np.array_equal(mwf_online_closed(mag, phase, A, 0), A * unit[:, None])


@pytest.mark.parametrize("forget", (1.0, 0.9))
def test_cuts_give_what_one_piece_gives(panned, forget):
    mag, phase, A, _ = panned
    T = mag.shape[1]
    whole, s_whole = mwf_online_em(mag, phase, A, 2, forget=forget)
    for cuts in ((1, 7, T - 8), (1,) * T):
        state, parts, t0 = None, [], 0
        for n in cuts:
            y, state = mwf_online_em(mag[:, t0:t0 + n], phase[:, t0:t0 + n], A[:, :, t0:t0 + n], 2, forget=forget, state=state)
            parts.append(y)
            t0 += n
        assert t0 == T
        assert np.array_equal(np.concatenate(parts, axis=2), whole)
        assert np.array_equal(state, s_whole)


def test_the_two_float64_restatements_agree_on_every_gpu_case():
    """Measured: at most 6e-13 of the mixture's peak at loading 1e-3 and 1e-2 (without loading, on masked estimates, up to 3e-2:
    those runs carry no oracle)."""
    worst = 0.0
    for name, c in gpu_cases().items():
        A = c["A"] / np.float32(c["pre_div"])
        peak = float(np.abs(mixture(c["mag"], c["phase"])).max())
        for niter, forget, loading, oracle in c["runs"]:
            if not oracle:
                continue
            y, _ = mwf_online_em(c["mag"], c["phase"], A, niter, forget, loading, c["eps"])
            y2 = mwf_online_closed(c["mag"], c["phase"], A, niter, forget, loading, c["eps"])
            assert np.isfinite(y).all() and np.isfinite(y2).all()
            err = float(np.abs(y - y2).max()) / peak
            worst = max(worst, err)
            assert err <= 1e-9, (run_key(name, niter, forget, loading), err)
    print("largest difference of the two float64 restatements: %.3g" % worst)


def test_estimates_sum_to_the_mixture(panned):
    # sum_j W_j = I - eps Cx^{-1}
    mag, phase, A, _ = panned
    X = mixture(mag, phase)
    for niter in (1, 2, 5):
        y, _ = mwf_online_em(mag, phase, A, niter)
        assert np.abs(y.sum(axis=1) - X).max() <= 1e-6 * np.abs(X).max(), niter


def test_the_filter_gains_at_least_6_db_on_panned_sources():
    """Measured: 11.3 dB against 2.15 dB of the unfiltered estimates (the batch filter of mwf_ref: 10.6 dB)."""
    mag, phase, A, img = make_case(4, 300, 65, seed=1)
    y0, _ = mwf_online_em(mag, phase, A, 0)
    y2, _ = mwf_online_em(mag, phase, A, 2, forget=1.0, loading=1e-3)
    before, after = sdr(y0, img), sdr(y2, img)
    print("SDR against the true images: unfiltered %.2f dB, online filter %.2f dB" % (before, after))
    assert after >= before + 6.0, (before, after)


def test_complex64_restatement_tracks_the_oracle(panned):
    # the precision yardstick of the GPU tests is the same recurrence, not another algorithm
    mag, phase, A, _ = panned
    y64, _ = mwf_online_em(mag, phase, A, 1)
    y32, _ = mwf_online_em(mag, phase, A, 1, precision="c64")
    assert y32.dtype == np.complex64
    assert np.abs(y32 - y64).max() <= 1e-4 * np.abs(mixture(mag, phase)).max()


def test_header_declares_and_library_exports_the_online_filter():
    names = _lib.header_symbols()
    assert set(SYMBOLS) <= set(names)
    lib = _lib.load()
    for n in SYMBOLS:
        assert getattr(lib, n).argtypes is not None, n
    assert lib.dcs_mwf_online_bytes(None) == -1 and lib.dcs_mwf_online_frames(None) == -1
    assert lib.dcs_mwf_online_destroy(None) == _lib.DCS_OK
    assert lib.dcs_mwf_online_reset(None) == _lib.DCS_EINVAL
    # the checks come before anything touches the context: no device is needed to see them
    h = ctypes.c_void_p()
    assert lib.dcs_mwf_online_create(None, 65, 3, 2, 1.0, 1e-3, 1e-10, ctypes.byref(h)) == _lib.DCS_EINVAL
    assert lib.dcs_mwf_online_push_f32(None, None, None, 0, None, 0, 0, 65, 1, 1.0, None, None) == _lib.DCS_EINVAL

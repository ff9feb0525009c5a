"""Properties of the multichannel Wiener filter's NumPy oracle (tests/mwf_ref.py), so that it cannot drift, and the
library's side of the contract that needs no GPU: the header declares ``dcs_mwf_f32`` and ``libdcs.so`` exports it."""
import numpy as np
import pytest

from deepconvsep_amd import _lib
from mwf_ref import make_case, mixture, mwf_em

PANNED = ((3, 37, 70), (4, 130, 65))


@pytest.fixture(scope="module")
def cases():
    out = {}
    for J, T, F in PANNED:
        out[(J, T, F, False)] = make_case(J, T, F, seed=1)
    out[(3, 37, 70, True)] = make_case(3, 37, 70, seed=1, dual_mono=True)
    return out


def test_zero_iterations_return_the_inputs(cases):
    for mag, phase, A, _ in cases.values():
        y = mwf_em(mag, phase, A, 0)
        assert np.array_equal(np.abs(y).astype(np.float32), A)
        unit = np.exp(1j * phase.astype(np.float64))
        assert np.allclose(y, A * unit[:, None], rtol=0, atol=1e-12 * A.max())


def test_estimates_sum_to_the_mixture(cases):
    # sum_j W_j = I - eps Cx^{-1}
    for key, (mag, phase, A, _) in cases.items():
        X = mixture(mag, phase)
        for niter in (1, 2, 5):
            y = mwf_em(mag, phase, A, niter)
            assert np.isfinite(y).all(), (key, niter)
            assert np.abs(y.sum(axis=1) - X).max() <= 1e-6 * np.abs(X).max(), (key, niter)


def test_error_against_the_true_images_falls_on_panned_sources(cases):
    for J, T, F in PANNED:
        mag, phase, A, img = cases[(J, T, F, False)]
        mse = [float(np.mean(np.abs(mwf_em(mag, phase, A, n) - img) ** 2)) for n in (0, 1, 2)]
        assert mse[0] > mse[1] > mse[2], mse


def test_complex64_restatement_tracks_the_oracle(cases):
    # the precision yardstick of the GPU tests is the same recurrence, not another algorithm
    for key, (mag, phase, A, _) in cases.items():
        y64, y32 = mwf_em(mag, phase, A, 1), mwf_em(mag, phase, A, 1, precision="c64")
        assert y32.dtype == np.complex64
        assert np.abs(y32 - y64).max() <= 1e-4 * np.abs(mixture(mag, phase)).max(), key


def test_header_declares_and_library_exports_the_filter():
    names = _lib.header_symbols()
    assert "dcs_mwf_f32" in names and "dcs_mwf_frames_per_block" in names
    lib = _lib.load()
    assert hasattr(lib, "dcs_mwf_f32")
    assert lib.dcs_mwf_frames_per_block() >= 1

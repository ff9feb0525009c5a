"""BSS Eval without a GPU: the float64 restatement (tests/bsseval_ref.py) against closed forms, and the host logic of
deepconvsep_amd/evaluation.py (energies -> dB, NaN / inf rules, permutation, framewise window count)."""
import numpy as np
import pytest

import bsseval_ref as ref
from deepconvsep_amd import evaluation as ev

T, FLEN = 1 << 17, 64


def _sources(n, seed, tail=FLEN):
    """white Gaussian sources whose last `tail` samples are zero (so a short FIR of them fits in T)"""
    s = np.random.default_rng(seed).standard_normal((n, T))
    s[:, T - tail:] = 0.0
    return s


def test_restatement_perfect_estimate_is_above_100_db():
    s = _sources(3, 0)
    for v in ref.bss_eval_sources(s, s, FLEN)[:3]:
        assert np.all(v >= 100.0), v
    for v in ref.bss_eval_images(s[:, :, None], s[:, :, None], FLEN)[:4]:
        assert np.all(v >= 100.0), v


def test_restatement_fir_distortion():
    s = _sources(3, 1)
    h = np.random.default_rng(2).standard_normal(48)
    e = np.array([np.convolve(x, h)[:T] for x in s])
    for v in ref.bss_eval_sources(e, s, FLEN)[:3]:
        assert np.all(v >= 100.0), v
    isr = ref.bss_eval_images(e[:, :, None], s[:, :, None], FLEN)[1]
    want = [10 * np.log10((x @ x) / ((y - x) @ (y - x))) for x, y in zip(s, e)]
    np.testing.assert_allclose(isr, want, rtol=0, atol=1e-6)


def test_restatement_interference_and_noise():
    s = _sources(3, 3)
    g = 0.1
    e = s.copy()
    e[0] = s[0] + g * s[1]
    sir = ref.bss_eval_sources(e, s, FLEN)[1]
    assert abs(sir[0] - 10 * np.log10((s[0] @ s[0]) / (g * g * (s[1] @ s[1])))) < 0.01
    n = 0.05 * np.random.default_rng(4).standard_normal(T)
    e = s.copy()
    e[2] = s[2] + n
    sar = ref.bss_eval_sources(e, s, FLEN)[2]
    assert abs(sar[2] - 10 * np.log10((s[2] @ s[2]) / (n @ n))) < 0.05


def test_db_from_restatement_energies_matches_its_time_domain_criteria():
    rng = np.random.default_rng(5)
    s = rng.standard_normal((3, 1 << 14, 2))
    e = s[[1, 0, 2]] + 0.3 * s[[2, 2, 0]] + 0.2 * rng.standard_normal(s.shape)
    en, crit = ref.images_pairs(e, s, 32)
    sdr, isr, sir, sar = ev.criteria_from_energies(en, images=True)
    for got, name in ((sdr, "SDR"), (isr, "ISR"), (sir, "SIR"), (sar, "SAR")):
        np.testing.assert_allclose(got, crit[name], rtol=0, atol=1e-9, err_msg=name)
    en, crit = ref.images_pairs(e[:, :, :1], s[:, :, :1], 32)
    sdr, isr, sir, sar = ev.criteria_from_energies(en, images=False)
    assert isr is None
    for got, name in ((sdr, "sSDR"), (sir, "sSIR"), (sar, "sSAR")):
        np.testing.assert_allclose(got, crit[name], rtol=0, atol=1e-9, err_msg=name)


def test_permutation_is_matlabs_winner():
    assert ev.matlab_perms(3) == [(2, 1, 0), (2, 0, 1), (1, 2, 0), (1, 0, 2), (0, 2, 1), (0, 1, 2)]
    sir = np.array([[1.0, 9.0, 0.0], [9.0, 1.0, 0.0], [0.0, 0.0, 5.0]])      # sir[jest, jtrue]
    assert list(ev.choose_perm(sir)) == [1, 0, 2]
    # a tie: every permutation has the same mean; MATLAB keeps the first, perms' [n .. 1]
    assert list(ev.choose_perm(np.ones((3, 3)))) == [2, 1, 0]
    assert list(ev.choose_perm(np.ones((2, 2)))) == [1, 0]
    # NaN means are ignored; all NaN -> the first permutation
    sir = np.array([[5.0, np.nan], [0.0, 1.0]])
    assert list(ev.choose_perm(sir)) == [0, 1]
    assert list(ev.choose_perm(np.full((2, 2), np.nan))) == [1, 0]
    # a perfect estimate has SIR +inf (a zero denominator): every permutation holding it would tie at +inf
    sir = np.array([[np.inf, -40.0, -35.0], [-38.0, np.inf, -41.0], [-33.0, -39.0, np.inf]])
    assert list(ev.choose_perm(sir)) == [0, 1, 2]
    for trial in range(20):
        m = np.random.default_rng(trial).integers(0, 3, (4, 4)).astype(float)
        assert list(ev.choose_perm(m)) == list(ref.best_perm(m))


def test_framewise_count_is_matlabs_formula_without_the_overrunning_window():
    for nsampl, win, ove in [(100, 30, 15), (1000, 300, 150), (44100 * 240, 30 * 44100, 15 * 44100), (59, 30, 15),
                             (44, 30, 15), (45, 30, 15), (30, 30, 15), (31, 30, 7)]:
        matlab = (nsampl - win + 1 + ove) // ove
        n = ev.framewise_count(nsampl, win, ove)
        assert n in (matlab, matlab - 1)
        assert (n - 1) * ove + win <= nsampl and n * ove + win > nsampl
    assert ev.framewise_count(44, 30, 15) == 1        # MATLAB's formula says 2; the second window would overrun
    assert ev.framewise_count(29, 30, 15) == 0        # nsampl < win: no windows (the formula says 1)
    assert ev.framewise_count(0, 30, 15) == 0


def test_nan_and_inf_rules():
    en = np.zeros((2, 1, 5))
    en[0, 0] = [1.0, 1.0, 1.0, 1.0, 0.0]            # perfect: e = s, every denominator 0
    en[1, 0] = [1.0, 0.0, 0.0, 0.0, 1.0]            # silent reference
    sdr, isr, sir, sar = ev.criteria_from_energies(en, images=True)
    assert sdr[0] == np.inf and isr[0] == np.inf and sir[0] == np.inf and sar[0] == np.inf
    assert all(np.isnan(v[1]) for v in (sdr, isr, sir, sar))
    en = np.array([[[0.0, 1.0, 0.0, 0.0, 0.0]]])     # silent estimate
    assert all(np.isnan(v[0]) for v in ev.criteria_from_energies(en, images=False) if v is not None)
    en = np.array([[[1.0, 1.0, 0.0, 0.0, 1.0]]])     # an estimate orthogonal to everything: SAR -inf, SIR NaN-free
    sdr, isr, sir, sar = ev.criteria_from_energies(en, images=True)
    assert sar[0] == -np.inf and sdr[0] == pytest.approx(-10 * np.log10(2.0))


def test_evaluation_is_exported():
    import deepconvsep_amd as dcs
    assert dcs.bss_eval is ev.bss_eval and dcs.bss_eval_images is ev.bss_eval_images
    assert dcs.bss_eval_sources is ev.bss_eval_sources

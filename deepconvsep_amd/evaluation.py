"""BSS Eval v3 separation quality on the MI355X: ``bss_eval_sources``, ``bss_eval_images`` and the framewise ``bss_eval``.

The reference scores its separations in MATLAB (evaluation/bss_eval/bss_eval_sources.m and bss_eval_images.m, called by
evaluation/evaluate_SS_iKala.m, Bach10_eval_only.m and, window by window, by the ``bss_eval`` of DSD100_eval_only.m).
Here the device computes five energies per (window, estimate, true source, channel) in float64 (``dcs_bss_energies``,
csrc/bsseval.hip); this module turns them into dB values, applies the degenerate-case rules and picks the permutation.

Degenerate cases (DESIGN.md "BSS Eval"):
  * a (source, window) whose reference image or estimate is all zeros gets NaN for every metric;
  * a denominator that is exactly 0 gives +inf;
  * a zero or numerically dependent reference channel leaves the span (the device drops a Cholesky pivot
    <= N * eps * max(diag G)) and does not affect the other sources;
  * values above about 100 dB are limited by rounding, as in the reference.

``perm`` is 0-based: estimate ``perm[j]`` is the one matched with true source ``j``.
"""
import ctypes
import itertools

import numpy as np

from . import _lib

FLEN = 512          # distortion filter length of the reference (bss_eval_sources.m / bss_eval_images.m)

SIR_CEILING = 10.0 * np.log10(1.0 / np.finfo(np.float64).eps)   # 156.5 dB: float64 energies resolve no more

# energy columns of dcs_bss_energies
E_EST, E_TRUE, E_CROSS, E_PROJ_J, E_RESID_ALL = range(5)


def framewise_count(nsampl, win, ove):
    """Windows of the framewise ``bss_eval``: MATLAB's ``floor((nsampl - win + 1 + ove) / ove)``, without a last window
    that would run past the end (MATLAB raises an index error there), and none when ``nsampl < win``."""
    nsampl, win, ove = int(nsampl), int(win), int(ove)
    if win < 1 or ove < 1:
        raise ValueError("bss_eval: win and ove must be positive (got %d, %d)" % (win, ove))
    if nsampl < win:
        return 0
    n = (nsampl - win + 1 + ove) // ove
    while n > 0 and (n - 1) * ove + win > nsampl:
        n -= 1
    return n


def matlab_perms(n):
    """``perms(1:n) - 1``: every permutation, in reverse lexicographic order."""
    return list(reversed(list(itertools.permutations(range(n)))))


def choose_perm(sir):
    """The permutation of bss_eval_sources / bss_eval_images: ``sir[jest, jtrue]``; maximise the mean over true sources
    of ``sir[perm[j], j]``.  The first maximum in ``perms`` order wins; NaN means are ignored (MATLAB's ``max``), and when
    every mean is NaN the first permutation is taken.  Values above ``SIR_CEILING`` dB count as ``SIR_CEILING`` here: they
    are rounding-limited, and an exactly zero denominator (+inf) would otherwise tie every permutation that contains it."""
    sir = np.minimum(np.asarray(sir, dtype=np.float64), SIR_CEILING)      # NaN stays NaN
    n = sir.shape[0]
    best, best_val = None, None
    for p in matlab_perms(n):
        s = 0.0
        for j in range(n):
            s += float(sir[p[j], j])
        m = s / n
        if np.isnan(m):
            if best is None:
                best = p
            continue
        if best_val is None or m > best_val:
            best, best_val = p, m
    return np.array(best, dtype=np.int64)


def _db(num, den):
    """10 log10(num / den) elementwise: den == 0 -> +inf."""
    num = np.asarray(num, dtype=np.float64)
    den = np.asarray(den, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        out = 10.0 * np.log10(num / den)
    return np.where(den == 0.0, np.inf, out)


def criteria_from_energies(en, images=True):
    """en [..., nchan, 5] (the columns of dcs_bss_energies) -> SDR, ISR, SIR, SAR (ISR None when not ``images``), each
    [...], summed over the channels.  NaN where the reference or the estimate is all zeros."""
    en = np.asarray(en, dtype=np.float64)
    e2 = en[..., E_EST]
    s2 = en[..., E_TRUE]
    es = en[..., E_CROSS]
    pj = en[..., E_PROJ_J]
    res = en[..., E_RESID_ALL]
    pall = e2 - res                                 # ||P_all e||^2
    S2, E2, PJ, PALL, RES = (x.sum(axis=-1) for x in (s2, e2, pj, pall, res))
    interf = np.maximum((pall - pj).sum(axis=-1), 0.0)
    sar = _db(PALL, RES)
    sir = _db(PJ, interf)
    if images:
        sdr = _db(S2, np.maximum((e2 - 2.0 * es + s2).sum(axis=-1), 0.0))
        isr = _db(S2, np.maximum((pj - 2.0 * es + s2).sum(axis=-1), 0.0))
    else:
        sdr = _db(PJ, np.maximum((e2 - pj).sum(axis=-1), 0.0))
        isr = None
    dead = (S2 == 0.0) | (E2 == 0.0)
    out = []
    for v in (sdr, isr, sir, sar):
        if v is not None:
            v = np.where(dead, np.nan, v)
        out.append(v)
    return tuple(out)


def energies(ref, est, nchan, win=None, hop=None, nwin=1, flen=FLEN, all_pairs=True, ctx=None):
    """``dcs_bss_energies``.  ref [nsrc_ref * nchan, nsampl], est [nsrc_est * nchan, nsampl] (row = source * nchan +
    channel), float64.  Returns [nwin, nsrc_est, nsrc_ref, nchan, 5] (``all_pairs``) or [nwin, nsrc, nchan, 5]."""
    from .runtime import default_context
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    est = np.ascontiguousarray(est, dtype=np.float64)
    if ref.ndim != 2 or est.ndim != 2 or ref.shape[1] != est.shape[1]:
        raise ValueError("bss_eval: references %r and estimates %r must be [channels, samples] of one length"
                         % (ref.shape, est.shape))
    if ref.shape[0] % nchan or est.shape[0] % nchan:
        raise ValueError("bss_eval: %d / %d rows are not whole sources of %d channels" % (ref.shape[0], est.shape[0], nchan))
    nsrc_ref, nsrc_est = ref.shape[0] // nchan, est.shape[0] // nchan
    nsampl = ref.shape[1]
    win = nsampl if win is None else int(win)
    hop = max(win, 1) if hop is None else int(hop)
    shape = (nwin, nsrc_est, nsrc_ref, nchan, 5) if all_pairs else (nwin, nsrc_ref, nchan, 5)
    if nwin == 0:
        return np.zeros(shape)
    if not all_pairs and nsrc_est != nsrc_ref:
        raise ValueError("bss_eval: %d estimates for %d sources" % (nsrc_est, nsrc_ref))
    if nsampl == 0:
        raise ValueError("bss_eval: empty signals")
    ctx = ctx if ctx is not None else default_context()
    lib = _lib.load()
    ref_d = ctx.to_device(ref, np.float64)
    est_d = ctx.to_device(est, np.float64)
    out_d = ctx.empty(shape, np.float64)
    _lib.check(lib.dcs_bss_energies(ctx._h, ctypes.c_void_p(ref_d.data_ptr()), ctypes.c_void_p(est_d.data_ptr()),
                                    nsrc_ref, nsrc_est, nchan, nsampl, win, hop, int(nwin), int(flen), int(bool(all_pairs)),
                                    ctypes.c_void_p(out_d.data_ptr())))
    return ctx.to_host(out_d)


def lagcorr(ref, est, flen=FLEN, ctx=None):
    """``dcs_bss_lagcorr``: c[k, n, d + flen - 1] = sum_t ref[k, t + d] * z[n, t], z = rows of ref then est."""
    from .runtime import default_context
    ref = np.ascontiguousarray(ref, dtype=np.float64)
    est = np.ascontiguousarray(est, dtype=np.float64).reshape(-1, ref.shape[1])
    ctx = ctx if ctx is not None else default_context()
    lib = _lib.load()
    ref_d = ctx.to_device(ref, np.float64)
    est_d = ctx.to_device(est, np.float64) if est.shape[0] else None
    out_d = ctx.empty((ref.shape[0], ref.shape[0] + est.shape[0], 2 * flen - 1), np.float64)
    _lib.check(lib.dcs_bss_lagcorr(ctx._h, ctypes.c_void_p(ref_d.data_ptr()),
                                   ctypes.c_void_p(est_d.data_ptr() if est_d is not None else None), ref.shape[0],
                                   est.shape[0], ref.shape[1], int(flen), ctypes.c_void_p(out_d.data_ptr())))
    return ctx.to_host(out_d)


def _select(values, perm):
    """values[jest, jtrue] -> [values[perm[j], j] for j]"""
    return np.array([values[perm[j], j] for j in range(len(perm))])


def bss_eval_sources(se, s, flen=FLEN, ctx=None):
    """bss_eval_sources.m: se, s [nsrc, nsampl] (estimates, true sources).  Returns SDR, SIR, SAR [nsrc] ordered by true
    source, and ``perm`` (0-based: estimate perm[j] goes with true source j), the permutation of best mean SIR."""
    se, s = np.asarray(se, dtype=np.float64), np.asarray(s, dtype=np.float64)
    if se.ndim != 2 or se.shape != s.shape:
        raise ValueError("bss_eval_sources: estimates %r and sources %r must both be [nsrc, nsampl]" % (se.shape, s.shape))
    en = energies(s, se, 1, flen=flen, all_pairs=True, ctx=ctx)[0]        # [jest, jtrue, 1, 5]
    sdr, _, sir, sar = criteria_from_energies(en, images=False)
    perm = choose_perm(sir)
    return _select(sdr, perm), _select(sir, perm), _select(sar, perm), perm


def bss_eval_images(ie, i, flen=FLEN, ctx=None):
    """bss_eval_images.m: ie, i [nsrc, nsampl, nchan] (estimated and true images).  Returns SDR, ISR, SIR, SAR [nsrc]
    ordered by true source, and the 0-based ``perm`` of best mean SIR."""
    ie, i = np.asarray(ie, dtype=np.float64), np.asarray(i, dtype=np.float64)
    if ie.ndim != 3 or ie.shape != i.shape:
        raise ValueError("bss_eval_images: estimates %r and images %r must both be [nsrc, nsampl, nchan]" % (ie.shape, i.shape))
    nsrc, nsampl, nchan = i.shape
    rows = lambda x: x.transpose(0, 2, 1).reshape(nsrc * nchan, nsampl)
    en = energies(rows(i), rows(ie), nchan, flen=flen, all_pairs=True, ctx=ctx)[0]   # [jest, jtrue, nchan, 5]
    sdr, isr, sir, sar = criteria_from_energies(en, images=True)
    perm = choose_perm(sir)
    return _select(sdr, perm), _select(isr, perm), _select(sir, perm), _select(sar, perm), perm


def bss_eval(ie, i, win, ove, flen=FLEN, ctx=None):
    """The framewise ``bss_eval`` of DSD100_eval_only.m: ie, i [nsampl, nchan, nsrc]; window k covers samples
    [k * ove, k * ove + win) and is scored as an isolated signal, estimate j against source j (no permutation).
    Returns SDR, ISR, SIR, SAR, each [nsrc, nwin] (nwin = :func:`framewise_count`; empty when nsampl < win)."""
    ie, i = np.asarray(ie, dtype=np.float64), np.asarray(i, dtype=np.float64)
    if ie.ndim != 3 or ie.shape != i.shape:
        raise ValueError("bss_eval: estimates %r and images %r must both be [nsampl, nchan, nsrc]" % (ie.shape, i.shape))
    nsampl, nchan, nsrc = i.shape
    nwin = framewise_count(nsampl, win, ove)
    if nwin == 0:
        return tuple(np.zeros((nsrc, 0)) for _ in range(4))
    rows = lambda x: x.transpose(2, 1, 0).reshape(nsrc * nchan, nsampl)
    en = energies(rows(i), rows(ie), nchan, win=win, hop=ove, nwin=nwin, flen=flen, all_pairs=False, ctx=ctx)
    sdr, isr, sir, sar = criteria_from_energies(en, images=True)   # [nwin, nsrc]
    return sdr.T.copy(), isr.T.copy(), sir.T.copy(), sar.T.copy()


def nanmedian(x):
    """The SiSEC summary of framewise values: the median over the windows, NaN ignored (NaN when nothing is left)."""
    x = np.asarray(x, dtype=np.float64)
    x = x[~np.isnan(x)]
    return float(np.median(x)) if x.size else float("nan")

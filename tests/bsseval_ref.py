"""Float64 NumPy restatement of BSS Eval v3, the reference's way: Gram matrix and cross terms of the delayed references
from zero-padded FFT correlations, ``np.linalg.solve`` over the channels left after silent ones and copies are dropped, the
projections synthesised as time signals, and every criterion from those signals.  It does not use the energy identities
of deepconvsep_amd/evaluation.py, so it checks them as well as the kernels.

Conventions as deepconvsep_amd.evaluation: ``perm`` 0-based (estimate perm[j] goes with true source j); NaN when the
reference or the estimate is all zeros; +inf for a zero denominator.
"""
import itertools

import numpy as np


def _nfft(n):
    return 1 << int(np.ceil(np.log2(max(n, 2))))


class _Spans(object):
    """The delayed copies r_k(t - a), a < flen, of the reference channels of one problem, and projections onto spans of
    subsets of them, in the zero-padded domain of length T + flen - 1."""

    def __init__(self, refs, flen):
        self.refs = np.asarray(refs, dtype=np.float64)     # [R, T]
        self.R, self.T = self.refs.shape
        self.L = flen
        self.nfft = _nfft(self.T + 2 * flen)
        self.F = np.fft.rfft(self.refs, self.nfft)

    def _corr(self, X, Y):
        """c(d) = sum_t x(t + d) y(t), d in (-L, L), for spectra X [.., nf], Y [.., nf] (broadcast) -> [.., 2L - 1]"""
        c = np.fft.irfft(X * np.conj(Y), self.nfft)
        L = self.L
        return np.concatenate([c[..., self.nfft - (L - 1):], c[..., :L]], axis=-1)

    def project(self, channels, ests):
        """orthogonal projections of the rows of ests [M, T] onto span{r_k(t - a): k in channels} -> [M, T + L - 1]"""
        L = self.L
        keep = []                                    # silent channels, and copies of a kept one (a mono source
        for k in channels:                           # duplicated to stereo), leave the span
            x = self.refs[k]
            xx = x @ x
            if xx == 0.0 or any((x @ self.refs[j]) ** 2 >= (1 - 1e-12) * xx * (self.refs[j] @ self.refs[j]) for j in keep):
                continue
            keep.append(k)
        M = ests.shape[0]
        out_len = self.T + L - 1
        if not keep:
            return np.zeros((M, out_len))
        Fk = self.F[keep]                                                # [K, nf]
        Fe = np.fft.rfft(ests, self.nfft)                                # [M, nf]
        K = len(keep)
        cc = self._corr(Fk[:, None, :], Fk[None, :, :])                  # [K, K, 2L - 1]: c_{k1,k2}(d)
        ce = self._corr(Fk[:, None, :], Fe[None, :, :])                  # [K, M, 2L - 1]
        a = np.arange(L)
        d = a[None, :] - a[:, None] + L - 1                              # b - a
        G = cc[:, :, d].transpose(0, 2, 1, 3).reshape(K * L, K * L)      # G[(k1,a),(k2,b)] = c_{k1,k2}(b - a)
        D = ce[:, :, L - 1 - a].transpose(0, 2, 1).reshape(K * L, M)     # D[(k,a),m] = c_{k,m}(-a)
        try:
            coef = np.linalg.solve(G, D)
        except np.linalg.LinAlgError:
            coef = np.linalg.lstsq(G, D, rcond=None)[0]
        coef = coef.reshape(K, L, M)
        Fc = np.fft.rfft(coef, self.nfft, axis=1)                        # [K, nf, M]
        P = np.fft.irfft(np.einsum("kf,kfm->mf", Fk, Fc), self.nfft)
        return P[:, :out_len]


def _db(num, den):
    if den == 0.0:
        return np.inf
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(num / den)


def images_pairs(ie, i, flen, pairs=None):
    """ie, i [nsrc, T, nchan].  Returns (energies [nsrc_est, nsrc, nchan, 5], criteria dict name -> [nsrc_est, nsrc]) for
    the images variant and the sources variant (meaningful when nchan == 1); ``pairs``: only these (jest, jtrue)."""
    ie = np.asarray(ie, dtype=np.float64)
    i = np.asarray(i, dtype=np.float64)
    nsrc, T, nchan = i.shape
    nest = ie.shape[0]
    L = flen
    refs = i.transpose(0, 2, 1).reshape(nsrc * nchan, T)
    ests = ie.transpose(0, 2, 1).reshape(nest * nchan, T)
    sp = _Spans(refs, L)
    P_all = sp.project(range(nsrc * nchan), ests)
    P_j = [sp.project(range(j * nchan, (j + 1) * nchan), ests) for j in range(nsrc)]
    pad = lambda x: np.concatenate([x, np.zeros(L - 1)])
    en = np.zeros((nest, nsrc, nchan, 5))
    names = ("SDR", "ISR", "SIR", "SAR", "sSDR", "sSIR", "sSAR")
    crit = {n: np.full((nest, nsrc), np.nan) for n in names}
    for jest in range(nest):
        for jtrue in range(nsrc):
            if pairs is not None and (jest, jtrue) not in pairs:
                continue
            acc = dict.fromkeys(("s", "all", "spat", "interf", "artif", "s_spat", "s_spat_interf", "pj", "pj_interf",
                                 "interf_artif"), 0.0)
            for c in range(nchan):
                m = jest * nchan + c
                e = pad(ests[m])
                s = pad(refs[jtrue * nchan + c])
                pj, pa = P_j[jtrue][m], P_all[m]
                e_spat, e_interf, e_artif = pj - s, pa - pj, e - pa
                en[jest, jtrue, c] = [e @ e, s @ s, e @ s, pj @ pj, e_artif @ e_artif]
                sq = lambda x: float(x @ x)
                acc["s"] += sq(s)
                acc["all"] += sq(e_spat + e_interf + e_artif)
                acc["spat"] += sq(e_spat)
                acc["interf"] += sq(e_interf)
                acc["artif"] += sq(e_artif)
                acc["s_spat"] += sq(s + e_spat)
                acc["s_spat_interf"] += sq(s + e_spat + e_interf)
                acc["pj"] += sq(pj)                                   # sources: s_true = P_j e
                acc["pj_interf"] += sq(pj + e_interf)
                acc["interf_artif"] += sq(e_interf + e_artif)
            dead = en[jest, jtrue, :, 1].sum() == 0.0 or en[jest, jtrue, :, 0].sum() == 0.0
            vals = {"SDR": _db(acc["s"], acc["all"]), "ISR": _db(acc["s"], acc["spat"]),
                    "SIR": _db(acc["s_spat"], acc["interf"]), "SAR": _db(acc["s_spat_interf"], acc["artif"]),
                    "sSDR": _db(acc["pj"], acc["interf_artif"]), "sSIR": _db(acc["pj"], acc["interf"]),
                    "sSAR": _db(acc["pj_interf"], acc["artif"])}
            for n in names:
                crit[n][jest, jtrue] = np.nan if dead else vals[n]
    return en, crit


def best_perm(sir):
    """max of the mean SIR over MATLAB's perms order (reverse lexicographic): first maximum, NaN means skipped, the
    first permutation when every mean is NaN"""
    n = sir.shape[0]
    perms = list(itertools.permutations(range(n)))[::-1]
    means = [sum(float(sir[p[j], j]) for j in range(n)) / n for p in perms]
    valid = [q for q, m in enumerate(means) if not np.isnan(m)]
    q = min(valid, key=lambda q: (-means[q], q)) if valid else 0
    return np.array(perms[q])


def bss_eval_sources(se, s, flen):
    """se, s [nsrc, T] -> SDR, SIR, SAR (by true source), perm"""
    se, s = np.asarray(se, dtype=np.float64), np.asarray(s, dtype=np.float64)
    _, c = images_pairs(se[:, :, None], s[:, :, None], flen)
    perm = best_perm(c["sSIR"])
    pick = lambda x: np.array([x[perm[j], j] for j in range(len(perm))])
    return pick(c["sSDR"]), pick(c["sSIR"]), pick(c["sSAR"]), perm


def bss_eval_images(ie, i, flen):
    """ie, i [nsrc, T, nchan] -> SDR, ISR, SIR, SAR (by true source), perm"""
    _, c = images_pairs(ie, i, flen)
    perm = best_perm(c["SIR"])
    pick = lambda x: np.array([x[perm[j], j] for j in range(len(perm))])
    return pick(c["SDR"]), pick(c["ISR"]), pick(c["SIR"]), pick(c["SAR"]), perm


def bss_eval(ie, i, win, ove, flen):
    """framewise, ie, i [T, nchan, nsrc] -> SDR, ISR, SIR, SAR [nsrc, nwin] (estimate j against source j)"""
    ie, i = np.asarray(ie, dtype=np.float64), np.asarray(i, dtype=np.float64)
    T, nchan, nsrc = i.shape
    nwin = 0 if T < win else (T - win + 1 + ove) // ove
    while nwin > 0 and (nwin - 1) * ove + win > T:
        nwin -= 1
    out = np.zeros((4, nsrc, nwin))
    for k in range(nwin):
        sl = slice(k * ove, k * ove + win)
        _, c = images_pairs(ie[sl].transpose(2, 0, 1), i[sl].transpose(2, 0, 1), flen,
                            pairs={(j, j) for j in range(nsrc)})
        for q, n in enumerate(("SDR", "ISR", "SIR", "SAR")):
            out[q, :, k] = np.diag(c[n])
    return tuple(out)


def lagcorr_int(ref, est, flen):
    """exact int64 lag correlations: c[k, n, d + flen - 1] = sum_t ref[k, t + d] z[n, t] (z = ref rows then est rows)"""
    ref = np.asarray(ref, dtype=np.int64)
    z = np.concatenate([ref, np.asarray(est, dtype=np.int64).reshape(-1, ref.shape[1])])
    R, T = ref.shape
    out = np.zeros((R, z.shape[0], 2 * flen - 1), dtype=np.int64)
    for di, d in enumerate(range(-(flen - 1), flen)):
        if d >= 0:
            out[:, :, di] = ref[:, d:] @ z[:, :T - d].T
        else:
            out[:, :, di] = ref[:, :T + d] @ z[:, -d:].T
    return out

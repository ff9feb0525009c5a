"""Float64 restatement of the sample-rate conversion ``dcs_resample_f32`` computes (include/dcs.h), sharing no code with the
package: the filter on the integer grid and a direct double loop, one dot product per output sample.

    up / down = fo / fi in lowest terms,  R = max(up, down) / rolloff,  H = ceil(Z R)
    h[t] = (up / R) sinc(t / R) I0(beta sqrt(1 - (t / (Z R))^2)) / I0(beta)      |t| <= Z R, else 0,   t = -H .. H
    y[m] = sum_n x[n] h[m down - n up],   0 <= n < L,  |m down - n up| <= H,   m = 0 .. ceil(L up / down) - 1
"""
import math

import numpy as np

PAIRS = [(48000, 44100), (22050, 44100), (32000, 44100), (96000, 44100), (16000, 44100), (8000, 44100), (44100, 48000)]
RATIOS = {(48000, 44100): (147, 160), (22050, 44100): (2, 1), (32000, 44100): (441, 320), (96000, 44100): (147, 320),
          (16000, 44100): (441, 160), (8000, 44100): (441, 80), (44100, 48000): (160, 147)}


def taps(up, down, zero_crossings=32, beta=12.0, rolloff=0.95):
    """(h float64 [2 H + 1], H)"""
    R = max(up, down) / rolloff
    width = zero_crossings * R
    H = int(np.ceil(width))
    t = np.arange(-H, H + 1, dtype=np.float64)
    inside = np.abs(t) <= width
    arg = np.where(inside, 1.0 - (t / width) ** 2, 0.0)
    h = (up / R) * np.sinc(t / R) * np.i0(beta * np.sqrt(arg)) / np.i0(beta)
    return np.where(inside, h, 0.0), H


def length(L, up, down):
    return -((-L * up) // down)


def tap_range(m, L, up, down, H):
    """[n_lo, n_hi] of the n with 0 <= n < L and |m down - n up| <= H (empty when n_lo > n_hi)"""
    n_lo = max(0, -((H - m * down) // up))            # ceil((m down - H) / up)
    n_hi = min(L - 1, (m * down + H) // up)
    return n_lo, n_hi


def resample(x, up, down, h, H, want_bound=False):
    """x float64 [L] -> y float64 [ceil(L up / down)]; with ``want_bound`` also, per output, the number of taps K and
    sum_n |x[n]| |h[m down - n up]|."""
    x = np.asarray(x, dtype=np.float64)
    L = x.shape[0]
    M = length(L, up, down)
    y = np.zeros(M)
    K = np.zeros(M, dtype=np.int64)
    mass = np.zeros(M)
    for m in range(M):
        n_lo, n_hi = tap_range(m, L, up, down, H)
        if n_hi < n_lo:
            continue
        n = np.arange(n_lo, n_hi + 1)
        hm = h[m * down - n * up + H]
        y[m] = np.dot(x[n_lo:n_hi + 1], hm)
        K[m] = n.size
        mass[m] = np.dot(np.abs(x[n_lo:n_hi + 1]), np.abs(hm))
    return (y, K, mass) if want_bound else y


def lowest_terms(fi, fo):
    g = math.gcd(fi, fo)
    return fo // g, fi // g

"""Shared by tests/test_follow_cpu.py, tests/test_gpu_follow.py and tests/test_gpu_stream_follow.py (test infrastructure): the
contract of csrc/follow.hip (include/dcs.h, "score following") restated in NumPy -- online dynamic time warping over a moving
window, one row per audio frame -- a brute-force enumeration that pins the restatement on small cases, and the onset error of
a position track on the synthetic piece of tests/align_ref.py.
"""
import itertools
import math

import numpy as np

import align_ref


def costs(a, S, dtype=np.float64):
    """c[u] = 1 - sum_k a[k] S[u][k], term by term in ``dtype`` (the way ``align_ref.dtw`` emulates the order of the sums)"""
    acc = np.zeros(S.shape[0], dtype=dtype)
    for k in range(S.shape[1]):
        acc = acc + a[k] * S[:, k]
    return (dtype(1) - acc).astype(dtype)


def follow(A, S, W, K, back, lam, dtype=np.float64, forced=None):
    """The follower on audio rows ``A [T, 12]`` and score rows ``S [U, 12]``.  Returns a dict:
    ``pos`` int32 ``[T]``; ``q`` int64 ``[T]`` the lowest cell of each row's minimum; ``rows`` ``[T, U]`` the row after every
    frame (minimum subtracted, +inf outside the window); ``w0`` int64 ``[T]`` the window start AFTER every frame; ``msum``
    ``[T]`` float64, the running sum of the minima ``m``; ``p`` the last position.
    ``forced``: the decisions ``q`` of another run (the device's), taken instead of this run's own; ``gap [T]`` then reports
    ``D'[forced[t]] - m`` per frame, how far from this run's minimum the forced cell was."""
    A = np.asarray(A, dtype=dtype)
    S = np.asarray(S, dtype=dtype)
    T, U = A.shape[0], S.shape[0]
    inf, lam = dtype(np.inf), dtype(lam)
    D = np.full(U, inf, dtype=dtype)
    w0, p, total = 0, 0, 0.0
    out = dict(pos=np.zeros(T, np.int32), q=np.zeros(T, np.int64), rows=np.full((T, U), inf, dtype=dtype),
               w0=np.zeros(T, np.int64), msum=np.zeros(T, np.float64), gap=np.zeros(T, np.float64))
    for t in range(T):
        c = costs(A[t], S, dtype)
        Dn = np.full(U, inf, dtype=dtype)
        if t == 0:
            Dn[0] = c[0]
        else:
            best = np.full(U, inf, dtype=dtype)
            best[1:] = D[:-1]
            best = np.minimum(best, (D + lam).astype(dtype))
            for k in range(2, K + 1):
                if k < U:
                    best[k:] = np.minimum(best[k:], (D[:-k] + lam).astype(dtype))
            hi = min(U, w0 + W)
            Dn[w0:hi] = (c[w0:hi] + best[w0:hi]).astype(dtype)
        m = Dn.min()
        assert np.isfinite(m), (t, w0)
        q = int(np.argmin(Dn))                                   # the lowest index that attains the minimum
        if forced is not None:
            out["gap"][t] = float(Dn[int(forced[t])]) - float(m)
            q = int(forced[t])
            m = Dn[q]
        p = max(p, q)
        D = (Dn - m).astype(dtype)
        total += float(m)
        w0 = max(w0, max(0, min(q - back, U - W)))
        D[:w0] = inf
        out["pos"][t], out["q"][t], out["w0"][t], out["msum"][t] = p, q, w0, total
        out["rows"][t] = D
    out["p"] = p
    return out


def window(row, w0, W):
    """what ``dcs_follow_row`` copies out: ``[W]`` with cell ``w0 + i`` at ``i``, +inf past the score's end"""
    out = np.full(W, np.inf, dtype=row.dtype)
    n = max(0, min(W, len(row) - w0))
    out[:n] = row[w0:w0 + n]
    return out


def brute_force(A, S, K, lam):
    """min over every step sequence in {0 .. K}^(T-1) from u = 0 of the summed cost, a step other than 1 costing ``lam``:
    float64 ``[U]``, +inf where no sequence ends"""
    A = np.asarray(A, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    T, U = A.shape[0], S.shape[0]
    c = 1.0 - A @ S.T
    best = np.full(U, np.inf)
    for steps in itertools.product(range(K + 1), repeat=T - 1):
        u, total = 0, c[0, 0]
        for t, s in enumerate(steps, start=1):
            u += s
            if u >= U:
                break
            total += c[t, u] + (0.0 if s == 1 else lam)
        else:
            best[u] = min(best[u], total)
    return best


def time_map(pos, U):
    """score frame u -> the first audio frame t with pos[t] >= u; past the last position reached, nominal tempo:
    (T - 1) + (u - pos[T-1]).  float64 ``[U]`` -- the restatement of ``align.follow_time_map``"""
    pos = np.asarray(pos, dtype=np.int64)
    out = np.zeros(U)
    for u in range(U):
        hit = np.nonzero(pos >= u)[0]
        out[u] = hit[0] if hit.size else (len(pos) - 1) + (u - int(pos[-1]))
    return out


def warped_onset_errors(pos, scores, U):
    """the same for the onsets ``align.follow_scores`` writes: the time map interpolated linearly at ``on fps`` between the
    score frames on either side (``align.warp_times``), restated"""
    tmap = time_map(pos, U)
    err = []
    for on, _, _ in scores:
        x = np.asarray(on, dtype=np.float64) * align_ref.FPS
        err.append(np.abs(np.interp(x, np.arange(U, dtype=np.float64), tmap) - align_ref.audio_time(on) * align_ref.FPS))
    return np.concatenate(err)


def onset_errors(pos, scores, U):
    """|first t with pos[t] >= ceil(on fps) - true audio onset| in frames, all instruments of the synthetic piece"""
    tmap = time_map(pos, U)
    err = []
    for on, _, _ in scores:
        u = np.minimum(np.ceil(np.asarray(on, dtype=np.float64) * align_ref.FPS).astype(np.int64), U - 1)
        err.append(np.abs(tmap[u] - align_ref.audio_time(on) * align_ref.FPS))
    return np.concatenate(err)

"""Shared by tests/test_align_cpu.py and tests/test_gpu_align.py (test infrastructure): the float64 restatement of
csrc/align.hip -- chroma of a magnitude spectrogram, dynamic time warping with the kernel's recursion, tie rule and band rule
-- a brute-force enumeration that pins that restatement on small matrices, and the seeded synthetic piece of the end-to-end
test with its float64 oracle run.
"""
import functools
import math

import numpy as np

from oracle import stft_np

FRAME, HOP, RATE = 2048, 512, 44100
FPS = RATE / HOP
INSTRUMENTS = ("bassoon", "clarinet", "saxophone", "violin")
NAMES = ("C", "C#", "D", "Eb", "E", "F", "F#", "G", "Ab", "A", "Bb", "B")

# Onset error of the float64 oracle run on the synthetic piece (frames of 512 samples), measured with oracle_run() below and
# checked by tests/test_align_cpu.py; the unaligned score is off by a median of ORACLE_UNALIGNED_MEDIAN frames.  The optimal path
# strays ORACLE_MAX_STRAY score frames from the straight line at the most (the GPU test's band of 64 holds it).
ORACLE_MEDIAN, ORACLE_P90 = 0.512, 2.347          # T = 795, U = 688, 61 notes; the largest error is 14.2 frames
ORACLE_UNALIGNED_MEDIAN = 61.6
ORACLE_MAX_STRAY = 38


# ------------------------------------------------------------------------------------------------ chroma
def chroma(mag, classes, floor=1e-6):
    """float64 ``[T, 12]``: class sums of ``mag [T, F]``, rows over their Euclidean norm, uniform where the norm is not above floor"""
    mag = np.asarray(mag, dtype=np.float64)
    classes = np.asarray(classes)
    c = np.zeros((mag.shape[0], 12))
    for k in range(12):
        c[:, k] = mag[:, classes == k].sum(axis=1)
    n = np.sqrt((c * c).sum(axis=1))
    out = np.full_like(c, 1.0 / math.sqrt(12.0))
    live = n > floor
    out[live] = c[live] / n[live, None]
    return out


def score_chroma(scores, U, hop=HOP, rate=RATE, nharmonics=6, decay=0.7):
    """float64 restatement of ``align.score_chroma``, note by note"""
    fps = rate / hop
    acc = np.zeros((U, 12))
    for on, off, names in scores:
        for a, b, name in zip(on, off, names):
            midi = name_to_midi(name)
            for u in range(max(0, int(math.ceil(a * fps))), min(U, int(math.ceil(b * fps)))):
                for k in range(1, nharmonics + 1):
                    acc[u, (midi + int(math.floor(12 * math.log2(k) + 0.5))) % 12] += decay ** (k - 1)
    out = np.full((U, 12), 1.0 / math.sqrt(12.0))
    for u in range(U):
        n = math.sqrt(float((acc[u] ** 2).sum()))
        if n > 0:
            out[u] = acc[u] / n
    return out


def name_to_midi(name):
    """"Bb3" -> 58 (letter, accidental, one octave digit: the names this file writes)"""
    pc = NAMES.index(name[:-1])
    return pc + 12 * (int(name[-1]) + 1)


# ------------------------------------------------------------------------------------------------ DTW
def in_band(T, U, band):
    """bool ``[T, U]``: |u (T-1) - t (U-1)| <= band (T-1); band None: all"""
    if band is None:
        return np.ones((T, U), dtype=bool)
    t = np.arange(T, dtype=np.int64)[:, None]
    u = np.arange(U, dtype=np.int64)[None, :]
    return np.abs(u * (T - 1) - t * (U - 1)) <= band * (T - 1)


def dtw(A, S, band=None, dtype=np.float64):
    """The kernel's recursion in ``dtype``: c = 1 - A S^T; D[0,0] = c[0,0]; D[t,u] = c[t,u] + best with best = D[t-1,u-1]
    (code 0), replaced by D[t-1,u] (1) only if strictly smaller, then by D[t,u-1] (2) only if strictly smaller than the best
    so far; cells outside the band and neighbours outside the matrix +inf.  Anti-diagonal by anti-diagonal (every cell of
    one depends on the two before it only).  Returns (path [n, 2] int32 from (0, 0) to the end, or None when the end cell is
    +inf; D[T-1, U-1]; D)."""
    A = np.asarray(A, dtype=dtype)
    S = np.asarray(S, dtype=dtype)
    T, U = A.shape[0], S.shape[0]
    acc = np.zeros((T, U), dtype=dtype)
    for k in range(A.shape[1]):                              # term by term: every partial sum in dtype
        acc = acc + A[:, k:k + 1] * S[None, :, k]
    cost = (dtype(1) - acc).astype(dtype)
    ok = in_band(T, U, band)
    inf = dtype(np.inf)
    D = np.full((T + 1, U + 1), inf, dtype=dtype)            # D[t + 1, u + 1]: a border of +inf
    code = np.zeros((T, U), dtype=np.uint8)
    for d in range(T + U - 1):
        t = np.arange(max(0, d - U + 1), min(T - 1, d) + 1)
        u = d - t
        best = D[t, u].copy()
        cd = np.zeros(t.size, dtype=np.uint8)
        up, left = D[t, u + 1], D[t + 1, u]
        m = up < best
        best[m], cd[m] = up[m], 1
        m = left < best
        best[m], cd[m] = left[m], 2
        if d == 0:
            best[:] = 0
        val = (cost[t, u] + best).astype(dtype)
        val[~ok[t, u]] = inf
        D[t + 1, u + 1] = val
        code[t, u] = cd
    D = D[1:, 1:]
    if not D[-1, -1] < inf:
        return None, float(D[-1, -1]), D
    path = []
    t, u = T - 1, U - 1
    while True:
        path.append((t, u))
        if t == 0 and u == 0:
            break
        c = code[t, u]
        t, u = (t - 1, u - 1) if c == 0 else (t - 1, u) if c == 1 else (t, u - 1)
        assert t >= 0 and u >= 0
    return np.asarray(path[::-1], dtype=np.int32), float(D[-1, -1]), D


def path_cost(A, S, path):
    """float64 sum of c along a path"""
    A = np.asarray(A, dtype=np.float64)
    S = np.asarray(S, dtype=np.float64)
    return float((1.0 - (A[path[:, 0]] * S[path[:, 1]]).sum(axis=1)).sum())


def brute_force(cost, ok):
    """Every monotone path from (0, 0) through in-band cells, by enumeration (no recursion over D): Dmin[t, u] = the least
    cost of a path ending there, +inf where there is none.  Then the path the tie rule picks: from the end, the predecessor
    with the least Dmin, the diagonal one winning ties, then the upper one."""
    T, U = cost.shape
    Dmin = np.full((T, U), np.inf)

    def walk(t, u, total):
        if not ok[t, u]:
            return
        total = total + cost[t, u]
        if total < Dmin[t, u]:
            Dmin[t, u] = total
        for dt, du in ((1, 1), (1, 0), (0, 1)):
            if t + dt < T and u + du < U:
                walk(t + dt, u + du, total)

    walk(0, 0, 0.0)
    if not Dmin[-1, -1] < np.inf:
        return None, Dmin
    path, t, u = [], T - 1, U - 1
    while True:
        path.append((t, u))
        if t == 0 and u == 0:
            break
        best, step = np.inf, None
        for dt, du in ((1, 1), (1, 0), (0, 1)):
            if t - dt >= 0 and u - du >= 0 and (step is None or Dmin[t - dt, u - du] < best):
                best, step = Dmin[t - dt, u - du], (dt, du)
        t, u = t - step[0], u - step[1]
    return np.asarray(path[::-1], dtype=np.int32), Dmin


# ------------------------------------------------------------------------------------------------ inputs of the GPU tests
def dyadic_features(T, U, seed):
    """Entries from {0, 1/4, 1/2, 3/4, 1}, about 30 % kept: every product and partial sum of c and D is exact in float32, and
    ties are everywhere"""
    rs = np.random.RandomState(seed)

    def draw(n):
        return (rs.randint(0, 5, (n, 12)) * 0.25 * (rs.uniform(size=(n, 12)) < 0.3)).astype(np.float32)
    return draw(T), draw(U)


def unit_features(T, U, seed):
    """real-valued non-negative rows of unit norm, float32"""
    rs = np.random.RandomState(seed)

    def draw(n):
        x = rs.uniform(0, 1, (n, 12)) ** 3
        return (x / np.sqrt((x * x).sum(axis=1))[:, None]).astype(np.float32)
    return draw(T), draw(U)


# ------------------------------------------------------------------------------------------------ the synthetic piece
RATES = (1.25, 0.8, 1.4, 0.9)        # audio seconds per score second, over SEGMENT score seconds each
SEGMENT, LEAD_IN, SCORE_SECONDS, NOISE = 2.0, 0.3, 8.0, 1e-3


def audio_time(score_time):
    """the piecewise-linear tempo map of the piece"""
    x = np.asarray(score_time, dtype=np.float64)
    knots = np.arange(len(RATES) + 1) * SEGMENT
    values = LEAD_IN + np.concatenate(([0.0], np.cumsum(np.asarray(RATES) * SEGMENT)))
    return np.interp(x, knots, values)


@functools.lru_cache(maxsize=None)
def piece(seed=5):
    """(scores, audio): four instruments, each in its own octave, notes of 0.25 .. 0.7 s back to back over 8 s of score time;
    the audio plays them at the tempo map above, six harmonics with amplitudes 0.7^k, 5 ms fades, plus noise of 1e-3.
    ``scores``: one (on, off, names) per instrument, times float32-exact the way ``read_score`` delivers them."""
    rs = np.random.RandomState(seed)
    n_audio = int(math.ceil((float(audio_time(SCORE_SECONDS)) + 0.2) * RATE))
    audio = np.zeros(n_audio)
    scores = []
    for j in range(len(INSTRUMENTS)):
        on, off, names = [], [], []
        t = float(rs.uniform(0.0, 0.2))
        while True:
            dur = float(rs.uniform(0.25, 0.7))
            if t + dur > SCORE_SECONDS:
                break
            midi = 43 + 12 * j + int(rs.randint(0, 12))
            a, b = float(np.float32(round(t, 3))), float(np.float32(round(t + dur, 3)))
            on.append(a)
            off.append(b)
            names.append("%s%d" % (NAMES[midi % 12], midi // 12 - 1))
            n0, n1 = int(round(float(audio_time(a)) * RATE)), int(round(float(audio_time(b)) * RATE))
            x = np.arange(n1 - n0) / RATE
            f0 = 440.0 * 2.0 ** ((midi - 69) / 12.0)
            tone = sum(0.7 ** k * np.sin(2 * np.pi * (k + 1) * f0 * x + rs.uniform(0, 2 * np.pi)) for k in range(6))
            fade = np.minimum(1.0, np.minimum(np.arange(n1 - n0), np.arange(n1 - n0)[::-1]) / (0.005 * RATE))
            audio[n0:n1] += 0.08 * tone * fade
            t += dur
        scores.append((np.asarray(on), np.asarray(off), names))
    audio += NOISE * rs.standard_normal(n_audio)
    audio.setflags(write=False)
    return scores, audio


def onset_errors(aligned_onsets, scores):
    """|aligned onset - true audio onset| in frames, all instruments"""
    err = [np.abs(np.asarray(got) - audio_time(on)) * FPS for got, (on, _, _) in zip(aligned_onsets, scores)]
    return np.concatenate(err)


def score_frames(scores):
    end = max(float(off.max()) for _, off, _ in scores)
    return int(math.ceil(end * FPS)) + 1


@functools.lru_cache(maxsize=None)
def oracle_run(band=None):
    """The whole alignment in float64: NumPy STFT magnitudes, chroma, score chroma, DTW, time map, warped onsets.
    Returns dict(T, U, path, cost, errors, unaligned, stray)."""
    from deepconvsep_amd import align
    scores, audio = piece()
    mag = np.abs(stft_np.stft_norm(audio, np.hanning(FRAME), float(HOP), float(FRAME))) / math.sqrt(FRAME)
    A = chroma(mag, align.bin_classes(FRAME, RATE))
    U = score_frames(scores)
    S = score_chroma(scores, U)
    path, cost, _ = dtw(A, S, band=band)
    tmap = align.time_map(path, U)
    errors = onset_errors([align.warp_times(on, tmap, FPS) for on, _, _ in scores], scores)
    unaligned = onset_errors([on for on, _, _ in scores], scores)
    T = A.shape[0]
    stray = float(np.abs(path[:, 1] - path[:, 0] * (U - 1) / (T - 1)).max())
    return dict(T=T, U=U, path=path, cost=cost, errors=errors, unaligned=unaligned, stray=stray, A=A, S=S)

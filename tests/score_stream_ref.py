"""Reference statements for the SCORE stream of csrc/stream.hip (``dcs_stream_create_score``; test infrastructure).

``synth_table`` draws a seeded note table with the corner cases the mask kernel can get wrong, ``frame_masks`` is the per-frame
definition of include/dcs.h in NumPy float32 (one absolute frame at a time, window ``(0, +inf)``), ``sorted_rows`` /
``candidate_range`` restate the host's choice of the note rows a push looks at, and ``whole_file_score`` is the whole-file
computation the stream must reproduce: ``oracle.score_np.filterSpec`` -> tiles per channel through
``oracle.tiling_np.generate_overlapadd`` -> ``chanmask_ref`` on the score-informed mixture -> ``stft_np.compute_inverse``.
"""
import bisect

import numpy as np

from oracle import score_np, stft_np, tiling_np

import chanmask_ref
import stream_ref

FLOOR = np.float32(1e-18)


# ------------------------------------------------------------------------------------------------ the table
def synth_table(ninst, T, F, nharm=4, boundary=None, seed=0):
    """A seeded note table ``[ninst, rows, 2 nharm + 3]`` for a signal of ``T`` frames and ``F`` bins.  With three or more
    instruments it holds: an instrument with no notes (the last one); two overlapping notes of one instrument; a cell two
    instruments both play; a note starting at frame 0; a band with ``f1 == F``; zero-width slots (``(0, 0)`` and ``(f, f)``
    with ``f > 0``); a row with ``midi == 0`` whose frames and bands would otherwise count; a note whose end is exactly ``T``;
    a note that covers the frames ``boundary - 1 .. boundary + 1`` (``boundary``: a tile's first frame, default ``T // 2``); a
    row with fractional frame numbers.  Two instruments cannot both share a cell and leave one of them empty: the empty
    instrument is then left out.  One instrument gets the rows of instrument 0."""
    assert T >= 12 and F >= 16 and nharm >= 3
    rs = np.random.RandomState(4000 + seed)
    W = 2 * nharm + 3
    b = T // 2 if boundary is None else int(boundary)
    assert 1 <= b < T - 1

    def bands(k=nharm):
        """k non-empty bands inside [0, F), the other slots (0, 0)"""
        out = np.zeros(2 * nharm)
        for i in range(k):
            f0 = int(rs.randint(0, F - 1))
            out[2 * i:2 * i + 2] = (f0, min(F, f0 + int(rs.randint(1, 6))))
        return out

    def row(t0, t1, midi, pairs):
        return np.concatenate([[t0, t1, midi], pairs])

    shared = np.zeros(2 * nharm)
    shared[0:2] = (3, 7)                                          # the cell both instrument 0 and instrument 1 play
    first = bands(nharm - 1)
    first[2 * (nharm - 1):] = (F - 3, F)                          # a band that ends at the last bin
    zero_w = bands(1)
    zero_w[2:4] = (5, 5)                                          # a zero-width slot that counts (fe > 0) and paints nothing
    inst0 = [
        row(0, min(6, T), 60, shared + np.concatenate([[0, 0], bands(nharm - 1)[:2 * (nharm - 1)]])),   # starts at frame 0
        row(2, min(9, T), 64, first),                             # overlaps the first note
        row(1, T, 0, bands()),                                    # midi == 0: does not count
        row(b - 1, b + 2, 55, bands()),                           # across a tile boundary
        row(6.5, 9.25, 50, bands(2)),                             # fractional frames: [6, 9)
        row(4, 4, 52, bands()),                                   # no duration
    ]
    inst1 = [
        row(1, min(5, T), 62, shared.copy()),                     # the shared cell, frames 1 .. 4
        row(T - 4, T, 67, zero_w),                                # ends exactly at T
        row(b, b + 1, 70, bands(2)),
    ]
    tables = [inst0]
    if ninst >= 2:
        tables.append(inst1)
    for j in range(2, ninst):
        if j == ninst - 1:
            tables.append([])                                     # an instrument with no notes
        else:
            rows = []
            for _ in range(5):
                t0 = int(rs.randint(0, T - 2))
                rows.append(row(t0, min(T, t0 + int(rs.randint(1, 9))), int(rs.randint(40, 80)), bands(int(rs.randint(1, nharm + 1)))))
            tables.append(rows)
    P = max(len(t) for t in tables) + 1                           # an all-zero row at the end of every instrument
    notes = np.zeros((ninst, P, W))
    for j, rows in enumerate(tables):
        order = rs.permutation(len(rows))                         # the table is not sorted by time
        for i, r in enumerate(order):
            notes[j, i] = rows[r]
    return notes


# ------------------------------------------------------------------------------------------------ per-frame masks
def _counting_rows(notes):
    """(instrument, first frame, end frame, [(f0, f1), ...]) of every row that counts and paints something"""
    out = []
    for j in range(notes.shape[0]):
        for p in range(notes.shape[1]):
            n0, n1, midi = notes[j, p, 0], notes[j, p, 1], notes[j, p, 2]
            a = max(n0, 0.0)
            if not (midi > 0) or not (n1 - a > 0):
                continue
            t0, t1 = int(a), int(n1)
            pairs = []
            for fs, fe in zip(notes[j, p, 3::2], notes[j, p, 4::2]):
                if fe > 0 and t1 > t0 and int(fe) > int(fs):
                    pairs.append((int(fs), int(fe)))
            if pairs:
                out.append((j, t0, t1, pairs))
    return out


def frame_on(rows, ninst, t, F):
    """``on_j[t][:]`` from counting rows: ``[ninst, F]`` bool"""
    on = np.zeros((ninst, F), dtype=bool)
    for j, t0, t1, pairs in rows:
        if t0 <= t < t1:
            for f0, f1 in pairs:
                on[j, f0:f1] = True
    return on


def frame_masks(notes, t, F, normalise):
    """``M_j[t][:]`` for every instrument, ``[ninst, F]`` float32: the definition of include/dcs.h for ONE absolute frame"""
    ninst = notes.shape[0]
    rows = _counting_rows(notes)
    on = frame_on(rows, ninst, t, F)
    one = np.float32(1.0)
    if normalise == 'sum':
        v = np.where(on, one, FLOOR).astype(np.float32)
        total = v[0].copy()
        for j in range(1, ninst):
            total = (total + v[j]).astype(np.float32)
        return (v / total[None]).astype(np.float32)
    assert normalise == 'max'
    out = np.empty((ninst, F), dtype=np.float32)
    for j in range(ninst):
        mx = one if any(r[0] == j for r in rows) else FLOOR
        out[j] = np.where(on[j], np.float32(one / mx), np.float32(FLOOR / mx))
    return out


def all_frame_masks(notes, T, F, normalise):
    """``[ninst, T, F]`` float32, frame by frame"""
    return np.stack([frame_masks(notes, t, F, normalise) for t in range(T)], axis=1)


# ------------------------------------------------------------------------------------------------ the candidate rows of a push
def sorted_rows(notes):
    """the counting rows sorted by first frame (stable) -> (rows, first frames, running maximum of the end frames)"""
    rows = sorted(_counting_rows(notes), key=lambda r: r[1])
    t0 = [r[1] for r in rows]
    end_max, m = [], 0
    for r in rows:
        m = max(m, r[2])
        end_max.append(m)
    return rows, t0, end_max


def candidate_range(t0, end_max, a, b):
    """the index range [lo, hi) of the sorted rows that can cover a frame of [a, b): first frame below b, and no row before lo
    ending after a -- two binary searches"""
    hi = bisect.bisect_left(t0, b)
    lo = bisect.bisect_right(end_max, a)
    return min(lo, hi), hi


# ------------------------------------------------------------------------------------------------ the whole-file computation
def mix32(M, mag32, mixture):
    """the score-informed mixture in float32, in the order of include/dcs.h: ``M_0 mag`` or ``((x_0 + x_1) + ...)``"""
    x = (M * mag32[None]).astype(np.float32)
    if mixture == 'ch0':
        return x[0]
    acc = x[0].copy()
    for j in range(1, x.shape[0]):
        acc = (acc + x[j]).astype(np.float32)
    return acc


def whole_file_score(audio, N, h, tc, ov, tiler, conv, S, win, scale, notes, normalise, mixture, seed=0, p=None, mag=None,
                     phase=None):
    """-> dict(M [ninst, T, F] float32, tiles [n, ninst, tc, F] float32, mix [T, F] float32, p, est [S, T, F], pcm [S, L], T,
    n_tiles).  ``mag`` / ``phase`` (a device's own float32 rows) and ``p`` given: evaluated at those."""
    audio = np.asarray(audio, dtype=np.float64)
    L = audio.size
    X = stft_np.stft_norm(audio, win, float(h), float(N))
    T, F = X.shape
    if mag is None:
        mag = (np.abs(X) / np.sqrt(N)).astype(np.float32)
    if phase is None:
        phase = np.angle(X)
    mag32 = np.asarray(mag, dtype=np.float32)
    ninst = notes.shape[0]
    masks = score_np.filterSpec(mag32, notes, ninst, 0, T, None, normalise=normalise)               # [T, ninst F] float32
    M = np.ascontiguousarray(masks.reshape(T, ninst, F).transpose(1, 0, 2))
    inp = (M * (np.float32(scale) * mag32)[None]).astype(np.float32)
    n = len(tiling_np.tile_starts(T, tc, ov, tiler))
    chans = []
    for j in range(ninst):
        fb, n2 = tiling_np.generate_overlapadd(inp[j], F, tc, ov, max(n, 1), tiler)
        assert n2 == n
        chans.append(fb.reshape(-1, tc, F)[:n])
    tiles = np.stack(chans, axis=1).astype(np.float32) if n else np.zeros((0, ninst, tc, F), np.float32)
    if p is None:
        p = (np.stack([stream_ref.tile_p(k, S, tc, F, seed) for k in range(n)], axis=1) if n
             else np.zeros((S, 0, tc, F), np.float32))
    mix = mix32(M, mag32, mixture)
    est, _ = chanmask_ref.chanmask_ref(p, mix[None], ov, conv, n_frames=T)
    est = est[0]
    pcm = np.stack([stft_np.compute_inverse(est[s], np.asarray(phase, dtype=np.float64), N, h, win)[:L] for s in range(S)])
    return dict(M=M, tiles=tiles, mix=mix, p=p, est=est, pcm=pcm, T=T, n_tiles=n)

"""NumPy restatement of the score-informed trainer's data feed (test infrastructure): what ``ScoreFeatureWindows.gather`` /
``dcs_trainer_gather_score`` (train::gather_score_kernel, csrc/train_core.hip) must write, element for element.
dataset.py's LargeDatasetMask2 cuts a window (loadFile :383-488), paints ``filterSpec`` (:839-879) for it and
trainCNNrwc.py:309-320 multiplies: ``inputs[b, j] = mask_j * (scale * mixture)``, ``targets[b, j] = scale * source_j``, all in
float32, one rounding per product (feed_ref.py explains the scale product)."""
import numpy as np

from feed_ref import data_pattern  # noqa: F401


def masks_np(notes, start, tc, rows, F):
    """``filterSpec(mag [rows, F], notes, start, start + tc)`` of LargeDatasetMask2 restated: float32 ``[ninst, rows, F]``,
    filtered_j / sum_i filtered_i with filtered in {1e-18, 1}, the instruments added in order."""
    notes = np.asarray(notes, dtype=np.float64)
    ninst = notes.shape[0]
    stop = start + tc
    filtered = np.full((ninst, rows, F), 1e-18, dtype=np.float32)
    for j in range(ninst):
        for n in notes[j]:
            if not n[2] > 0:
                continue
            a, b = max(n[0], start), min(n[1], stop)
            if not b - a > 0:
                continue
            t0, t1 = max(int(a) - start, 0), min(int(b) - start, rows)
            for fs, fe in zip(n[3::2], n[4::2]):
                if fe > 0 and t1 > t0:
                    assert 0 <= int(fs) and int(fe) <= F
                    filtered[j, t0:t1, int(fs):int(fe)] = 1.0
    total = filtered[0].copy()
    for j in range(1, ninst):
        total = total + filtered[j]
    assert total.dtype == np.float32
    return filtered / total[None]


def gather_np(files, notes, table_rows, tc, F, scale):
    """``files``: arrays ``[1 + ninst, T_i, F]``; ``notes``: per file ``[ninst, P_i, W]``; ``table_rows``: (file, start) pairs,
    file -1 = a zero slot.  Returns float32 inputs and targets ``[B, ninst, tc, F]``; zero for file -1 and frames past T_i."""
    rows = np.asarray(table_rows, dtype=np.int64).reshape(-1, 2)
    ninst = np.asarray(notes[0]).shape[0]
    x = np.zeros((len(rows), ninst, tc, F), dtype=np.float32)
    t = np.zeros((len(rows), ninst, tc, F), dtype=np.float32)
    sc = np.float32(scale)
    for b, (fi, start) in enumerate(rows):
        if fi < 0:
            continue
        a = np.asarray(files[fi], dtype=np.float32)
        assert a.shape[0] == 1 + ninst and a.shape[2] == F
        n = max(0, min(tc, a.shape[1] - int(start)))
        w = sc * a[:, start:start + n, :]
        m = masks_np(notes[fi], int(start), tc, n, F)
        prod = m * w[0][None]
        assert w.dtype == np.float32 and prod.dtype == np.float32
        x[b, :, :n] = prod
        t[b, :, :n] = w[1:]
    return x, t


# The fixture's files (tests/golden/make_golden_train_si.py): (T, data offset, scale), time context 8, overlap 3, F 13.  The
# scales are powers of two: loadFile multiplies the float64 file by the scale and then narrows, the feed narrows the file first
# (feed_ref.py), and only a power of two makes the two the same float32 for every magnitude -- then the comparison with the
# reference's arrays is bit for bit (tests/test_train_edges_cpu.py shows the one ulp of any other scale on the mono feed).
TC, OVERLAP, F = 8, 3, 13
FILES = [(24, 0, 0.5), (5, 7, 0.25), (8, 3, 0.5)]


def _note(t0, t1, midi, bands, width=9):
    n = np.zeros(width)
    n[0], n[1], n[2] = t0, t1, midi
    for k, (f0, f1) in enumerate(bands):
        n[3 + 2 * k], n[4 + 2 * k] = f0, f1
    return n


def fixture_notes():
    """Per file ``[4, P, 9]`` (three harmonics).  File 0 (24 frames, windows at 0, 5, 10, 15): instrument 0 plays 0 .. 5 and
    4 .. 9 (the second starts before the window at 5 and ends inside it), instrument 1 plays 3 .. 12 and shares bin 3 with
    instrument 0 in frames 4 .. 8, instrument 2 plays 15 .. 18 and a note whose MIDI number is 0 (ignored), instrument 3 has
    no notes; nobody plays in frames 12 .. 14 and from 18 on (all masks 0.25).  File 1 is shorter than the time context (one
    padded window), file 2 exactly as long (one slot that loadFile never fills)."""
    f0 = np.zeros((4, 3, 9))
    f0[0, 0] = _note(0, 5, 60, [(1, 3), (6, 8)])
    f0[0, 1] = _note(4, 9, 62, [(2, 4), (7, 9), (11, 13)])
    f0[1, 0] = _note(3, 12, 55, [(3, 5), (9, 10)])
    f0[2, 0] = _note(15, 18, 70, [(0, 2), (5, 6)])
    f0[2, 1] = _note(16, 20, 0, [(8, 12)])
    f0[2, 2] = _note(20.5, 20.9, 71, [(8, 12)])     # no whole frame
    f1 = np.zeros((4, 2, 9))
    f1[0, 0] = _note(1, 4, 60, [(1, 3)])
    f1[3, 0] = _note(0, 30, 48, [(2, 6), (0, 0)])
    f1[3, 1] = _note(2, 3, 50, [(12, 13)])
    f2 = np.zeros((4, 1, 9))
    f2[1, 0] = _note(0, 8, 60, [(1, 3)])
    return [f0, f1, f2]


def fixture_files():
    return [data_pattern(4, T, F, offset) for T, offset, _ in FILES]

"""Seeded inputs of the score-informed score-render tests (test infrastructure): the pieces that
tests/golden/make_golden_score_render_si.py runs the reference's generator on and the tests run the project on, on top of
the tiny RWC tree and the scores of tests/score_render_ref.py.  Only the reference's answers are stored in
tests/golden/score_render_si.npz.

Sample rate 1000 Hz, 2 s chunks, frame 256 and hop 50: 1000 / 50 is a whole number, so the frame rate of ``expandMidi`` is
20 under either Python's division.  ``size`` is 2000 samples without shifts and 1800 with a largest shift of 0.2 s."""
import os

import numpy as np

import score_render_ref as R

SR, CHUNK, FRAME, HOP = R.SR, 2.0, 256, 50
NHARMONICS, INTERVAL, TUNING = 20, 50, 440
SHIFTS = (0., 0.1, 0.2)

# the ground-truth aligned scores <source>_g.txt of the main piece: the original ones, every note 30 ms late
SCORES_GT = {s: [(on + 0.03, off + 0.03, name) for on, off, name in notes] for s, notes in R.SCORES.items()}


def _with(source, notes):
    out = dict(R.SCORES)
    out[source] = notes
    return out


# piece -> the scores <source>_g_original.txt; one source differs from the main piece
PIECES = {
    R.PIECE: R.SCORES,
    # E4 is not in the tree: GetOutOfLoop in chunk 0, which skips that chunk only
    '02-Missing': _with('bassoon', [(0.05, 0.30, 'A3'), (0.40, 0.90, 'E4')] + R.SCORES['bassoon'][3:]),
    # one violin note in chunk 1: expandMidi selects fewer than two notes and the generator cannot go on
    '03-Single': _with('violin', [(0.00, 0.50, 'D4'), (0.55, 1.00, 'C#4'), (1.00, 1.60, 'Bb3'), (2.60, 3.00, 'B3'),
                                  (4.20, 4.90, 'C#4'), (4.90, 5.60, 'A3'), (5.60, 6.20, 'Bb3')]),
    # a clarinet note that begins at 1.86 s with three frames of audio: past size = 1800 with 100 samples left over
    '04-Past': _with('clarinet', [(0.30, 1.20, 'C4'), (1.20, 1.35, 'A3'), (1.86, 2.50, 'B3')] + R.SCORES['clarinet'][4:]),
    # clarinet notes at b == size (1.81 s, frame 36) and past it with nothing left over (1.86 s one frame, 1.91 s two
    # frames): the file is written without them
    '05-Edge': _with('clarinet', [(0.30, 1.20, 'C4'), (1.20, 1.35, 'A3'), (1.81, 1.86, 'D4'), (1.86, 1.91, 'A3'),
                                  (1.91, 2.50, 'B3')] + R.SCORES['clarinet'][4:]),
}

# (piece, style, combination of R.COMBOS, chunk) whose audio, tables and stem are recorded, and the case each must contain
RENDERS = (
    (R.PIECE, 'original', 1, 0),      # unequal shifts; a clarinet note cut at the end of the track
    (R.PIECE, 'gt', 0, 0),            # style gt; a later note overwrites an earlier one
    (R.PIECE, 'original', 2, 1),      # unequal shifts, a middle chunk
    (R.PIECE, 'original', 0, 2),      # the last chunk
    ('05-Edge', 'original', 1, 0),    # notes at and past size that paint nothing
)
# the pieces whose written (combination, chunk) pairs are recorded for combinations 0 and 1
WRITTEN = ('02-Missing', '03-Single', '04-Past', '05-Edge')
WRITTEN_COMBOS = (0, 1)
STYLE_MIDI = {'original': '_original', 'gt': ''}


def write_pieces(db):
    """The score tree ``<db>/<piece>/<source>_g_original.txt`` of every piece, and ``<source>_g.txt`` of the main one."""
    for piece, scores in PIECES.items():
        R.write_scores(db, piece, scores)
    R.write_scores(db, R.PIECE, SCORES_GT, style_midi='')
    return db


def overwrites(tracks):
    """True where some note of ``tracks`` begins inside an earlier note of its track."""
    return any(b2 < b1 + l1 for t in tracks for (b1, _, l1), (b2, _, _) in zip(t, t[1:]))


def stem_array(stem):
    return np.frombuffer(stem.encode('ascii'), dtype=np.uint8).copy()


def piece_dir(db, piece):
    return os.path.join(db, piece)

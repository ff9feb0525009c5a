"""Seeded inputs of the score-render tests (test infrastructure): a tiny RWC tree, Bach10-style score files and the
combinations that tests/golden/make_golden_score_render.py runs the reference on and the tests run the project on.  Only
the reference's answers are stored in tests/golden/score_render.npz; the inputs are rebuilt from here.

Sample rate 1000 Hz, so that a 2 s chunk is 2000 samples (about 34 frames at hop 64, 6 at hop 512).  Notes are
``synth_audio(n, seed, silence=False) * 0.25`` written as 16-bit wav: a mixture of four stays in the amplitude range the
float32 STFT bounds of tests/test_gpu_parity.py were established for."""
import os

import numpy as np

from deepconvsep_amd.separation import write_wav
from deepconvsep_amd.synth import synth_audio

SR = 1000
CHUNK = 2
INSTRUMENT_IDS = (30, 31, 27, 15)
SOURCES = ('bassoon', 'clarinet', 'saxophone', 'violin')
CASES, DYNAMICS, STYLES = (1, 2, 3), ('F', 'M', 'P'), ('NO',)
PITCHES = (57, 58, 59, 60, 61, 62)             # A3 Bb3 B3 C4 C#4 D4
LONG = 60                                      # the pitch whose samples last 1.7 s: a note can lie wholly inside it
TRIM_ID = 99                                   # an instrument whose notes begin with silence, for the onset trim
TRIM_LEADS = (0, 300, 1100, 1500, 2600)
TRIM_LONG = 3.5                                # s: longer than every onset plus 1024 samples, shorter than the notes
PIECE = '01-Test'

SCORES = {
    # two notes clamped to b = 0 under a shift of 0.2; overlap of consecutive notes under any shift; a silence of 1.35 s
    'bassoon': [(0.05, 0.30, 'A3'), (0.15, 0.50, 'B3'), (0.50, 0.75, 'D4'), (2.10, 2.60, 'C4'), (2.60, 3.30, 'A3'),
                (3.30, 3.95, 'Bb3'), (4.05, 4.50, 'B3'), (4.50, 5.20, 'C#4'), (5.20, 5.70, 'D4'), (5.70, 6.40, 'A3')],
    # two notes wholly inside the long C4; a note cut at the chunk's end; four notes of 80 ms (one frame touches 3 or more)
    'clarinet': [(0.30, 1.90, 'C4'), (0.60, 0.80, 'D4'), (1.20, 1.35, 'A3'), (1.70, 2.40, 'B3'), (2.40, 2.48, 'A3'),
                 (2.48, 2.56, 'Bb3'), (2.56, 2.64, 'B3'), (2.64, 2.72, 'C#4'), (2.72, 3.60, 'D4'), (3.60, 4.30, 'A3'),
                 (4.30, 5.00, 'C4'), (5.00, 5.70, 'Bb3'), (5.70, 6.30, 'D4')],
    # a first note that begins 40 samples into the signal: inside the first frame, after its zero padding
    'saxophone': [(0.04, 0.60, 'Bb3'), (0.60, 1.10, 'C#4'), (1.10, 1.72, 'A3'), (1.72, 2.30, 'B3'), (2.30, 3.00, 'C4'),
                  (3.00, 3.70, 'D4'), (3.70, 4.40, 'Bb3'), (4.40, 5.10, 'A3'), (5.10, 5.72, 'C#4'), (5.72, 6.35, 'B3')],
    # a note of 5 ms, which getMidi drops
    'violin': [(0.00, 0.50, 'D4'), (0.50, 0.505, 'A3'), (0.55, 1.00, 'C#4'), (1.00, 1.60, 'Bb3'), (1.60, 2.20, 'A3'),
               (2.20, 2.90, 'B3'), (2.90, 3.50, 'D4'), (3.50, 4.20, 'C4'), (4.20, 4.90, 'C#4'), (4.90, 5.60, 'A3'),
               (5.60, 6.20, 'Bb3')],
}

# (time shift, index of the dynamics, index of the style, player) per source
COMBOS = np.array([
    [[0.0, 0, 0, 1], [0.0, 1, 0, 2], [0.0, 2, 0, 3], [0.0, 0, 0, 2]],
    [[0.2, 0, 0, 1], [0.0, 1, 0, 1], [0.1, 2, 0, 2], [0.2, 1, 0, 3]],
    [[0.1, 2, 0, 3], [0.2, 0, 0, 2], [0.2, 1, 0, 1], [0.0, 2, 0, 1]],
], dtype=np.float64)
# the (combination, chunk, frame, hop) whose rendered audio is recorded; a block is recorded where frame is not 0
RENDERS = ((0, 0, 256, 64), (1, 0, 1024, 512), (2, 1, 0, 0), (1, 2, 0, 0))

SIB_LENGTHS = (500, 450, 560, 500)
SIB_SHIFTS, SIB_GAINS = (0., 0.1, 0.2), (1.,)
SIB_PICK = (0, 7)                               # the combinations of the 3 ** 4 - 3 = 78 whose audio is recorded
SIB_BLOCK = 1                                   # the one of them whose block at (4096, 512) is recorded (a block is 246 kB)


def _recording(instid, case, dyn, tag, pitches, leads=None):
    """One recording and its annotation: the notes one after the other, 40 samples of silence between them."""
    seed0 = 1000 * instid + 100 * case + 10 * DYNAMICS.index(dyn) + (7 if tag == 'YY' else 0)
    parts, starts, ends, at = [], [], [], 0
    for k, p in enumerate(pitches):
        rs = np.random.RandomState(seed0 + k)
        n = 1700 if p == LONG else int(rs.randint(250, 700))
        lead = 0
        if leads is not None:
            n, lead = 4000 + 100 * k, leads[k]
        x = synth_audio(n, seed=seed0 + k, silence=False) * 0.25
        parts += [np.zeros(lead), x, np.zeros(40)]
        starts.append(at)
        ends.append(at + lead + n)
        at += lead + n + 40
    return np.concatenate(parts), np.asarray(starts, dtype=np.float64), np.asarray(ends, dtype=np.float64)


def _write_recording(root, instid, case, dyn, tag='XX', style='NO', pitches=PITCHES, leads=None, mat=True):
    from scipy import io
    name = "%d%d%s%s%s.WAV" % (instid, case, tag, style, dyn)
    d = os.path.join(root, 'wav', "%d%d" % (instid, case))
    os.makedirs(d, exist_ok=True)
    os.makedirs(os.path.join(root, 'mat'), exist_ok=True)
    audio, starts, ends = _recording(instid, case, dyn, tag, pitches, leads)
    write_wav(os.path.join(d, name), audio, SR)
    if mat:
        # a struct whose fields stand where rwc.py reads them by position: 0 (a struct whose field 3 is the sample rate),
        # 3 dynamics, 4 instrument id, 6 name, 7 symbol, 9 style, 14 note numbers, 15 starts, 16 ends (in samples)
        fs = dict(info=dict(a=0, b=0, c=0, sampleRate=float(SR)), f1=0, f2=0, dynamics=dyn, instid=instid, f5=0,
                  instrumentName='instrument %d' % instid, instrumentSymbol=tag, f8=0, style=style, f10=0, f11=0, f12=0,
                  f13=0, nr=np.asarray(pitches), start=starts, end=ends)
        io.savemat(os.path.join(root, 'mat', name.lower() + '.mat'), dict(featureStruct=fs))
    return name


def write_rwc_tree(root):
    """The tree under ``root``: per instrument, player and dynamics one recording of the six pitches; for (30, 1, F) a second
    recording 'YY' of the same notes (the sorted listing takes 'XX'); a staccato recording that the style filter drops; a
    recording without annotation; and instrument 99 whose five notes begin with 0 .. 2600 samples of silence."""
    for instid in INSTRUMENT_IDS:
        for case in CASES:
            for dyn in DYNAMICS:
                _write_recording(root, instid, case, dyn)
    _write_recording(root, 30, 1, 'F', tag='YY')
    _write_recording(root, 30, 1, 'F', tag='ZZ', style='ST')
    _write_recording(root, 31, 2, 'M', tag='QQ', mat=False)
    _write_recording(root, TRIM_ID, 1, 'F', pitches=PITCHES[:len(TRIM_LEADS)], leads=TRIM_LEADS)
    return root


def write_scores(db, piece=PIECE, scores=SCORES, style_midi='_original'):
    d = os.path.join(db, piece)
    os.makedirs(d, exist_ok=True)
    for s, notes in scores.items():
        with open(os.path.join(d, s + '_g' + style_midi + '.txt'), 'w') as fh:
            for on, off, name in notes:
                fh.write("%.3f,%.3f,%s\n" % (on, off, name))
    return d


def sibelius_sources():
    return [synth_audio(L, seed=300 + i, silence=False) * 0.25 for i, L in enumerate(SIB_LENGTHS)]

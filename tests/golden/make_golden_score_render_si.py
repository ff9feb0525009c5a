"""Writes tests/golden/score_render_si.npz from the reference's own source.  CPU only; needs the reference tree
(DCS_REFERENCE_ROOT).

    python tests/golden/make_golden_score_render_si.py

Executed as written on the seeded inputs of tests/score_render_si_ref.py (the tiny RWC tree of tests/score_render_ref.py,
five pieces of score files, sample rate 1000 Hz, 2 s chunks, frame 256, hop 50), with the stand-ins of
make_golden_score_render.py and two more: ``str`` whose ``encode('base64', 'strict')`` is Python 2's codec, and
``transformFFT`` returning a ``tt`` that holds the frame and hop sizes and records what ``compute_transform`` and
``saveTensor`` are given:

* ``Engine.__init__`` (examples/bach10_scoreinformed/compute_features_bach10rwc.py:63-90) with ``np.random`` =
  ``RandomState(seed)`` for the four settings make_golden_score_render.py draws (``combos_*``);
* ``Engine.__call__`` (:96-163) for the (piece, style, combination, chunk) of ``RENDERS``: ``audio_<k> [size, 5]``,
  ``melody_g_<k>``, ``melody_e_<k>``, ``stem_<k>`` (the path below the feature directory without ``.data``, as bytes) and
  the length of every segment ``getAudio`` returned (``seglen_<k>``).  The generator checks here that the pairs hold the
  cases the tests name: unequal shifts, style gt, a later note overwriting an earlier one, a note cut at the end of the
  track, notes at and past ``size`` that paint nothing;
* for the pieces of ``WRITTEN`` and two combinations, the (combination, chunk) pairs for which ``compute_transform`` was
  called (``written_<piece>``) -- the pieces on which the reference writes no file for some of them.
"""
import base64
import itertools
import os
import re
import sys
import tempfile
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.dirname(HERE), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import make_golden_score_render as G  # noqa: E402
import score_render_ref as R  # noqa: E402
import score_render_si_ref as SI  # noqa: E402
from oracle import ref_exec  # noqa: E402

GEN = "examples/bach10_scoreinformed/compute_features_bach10rwc.py"


class _Str(str):
    def encode(self, codec='utf-8', errors='strict'):
        if codec == 'base64':
            return base64.encodebytes(str.encode(self, 'ascii')).decode('ascii')
        return str.encode(self, codec, errors)


class GetOutOfLoop(Exception):
    pass


class _TT(object):
    def __init__(self, log):
        self.frameSize, self.hopSize, self.log = SI.FRAME, SI.HOP, log

    def compute_transform(self, audio, path, phase=False):
        assert phase is False
        self.log.append(['m', path, np.array(audio, dtype=np.float64)])

    def saveTensor(self, t, suffix):
        self.log.append([suffix, None, np.array(t, dtype=np.float64)])


def engine_combos(time_shifts, dynamics, styles, cases, sample_size, seed):
    me = types.SimpleNamespace(allowed_dynamics=dynamics, allowed_styles=styles, allowed_case=cases,
                               sources=['bassoon', 'clarinet', 'saxophone', 'violin'])
    fake_np = types.SimpleNamespace(array=np.array, random=np.random.RandomState(seed))
    ns = dict(np=fake_np, it=itertools, xrange=range, self=me, time_shifts=list(time_shifts), sample_size=sample_size)
    G._run(GEN, 63, 90, ns)
    return np.asarray(me.combo, dtype=np.float64)


def call(util, instruments, db, piece, style, c):
    """:96-163 for the combination ``c`` on all chunks of the piece.  Returns the log of compute_transform / saveTensor
    calls, the segment lengths in call order, and the exception that ended it, if any."""
    log, seglen = [], []

    def recorded(plain):
        def getAudio(max_duration=0):
            a = plain(max_duration)
            seglen.append(len(a))
            return a
        return getAudio
    notes = [n for ins in instruments for n in ins.notes]
    for n in notes:
        n.getAudio = recorded(n.getAudio)
    me = types.SimpleNamespace(sources=list(R.SOURCES), sources_midi=list(R.SOURCES), sampleRate=SI.SR, style=style,
                               style_midi=SI.STYLE_MIDI[style], instruments=instruments, allowed_dynamics=list(R.DYNAMICS),
                               allowed_styles=list(R.STYLES), chunk_size=SI.CHUNK, db=os.path.join(db, piece),
                               feature_path=os.path.join('FEATURES', piece), nharmonics=SI.NHARMONICS, interval=SI.INTERVAL,
                               tuning_freq=SI.TUNING)
    u = types.SimpleNamespace(getMidiLength=util["getMidiLength"], getMidiNum=util["getMidiNum"], expandMidi=util["expandMidi"])
    ns = dict(np=np, os=os, util=u, str=_Str, transformFFT=lambda **kw: _TT(log), blackmanharris=None,
              GetOutOfLoop=GetOutOfLoop)
    # the script's sample rate is the constant 44100 (:47, :102, :128); here it is the tree's
    src = textwrap.dedent(ref_exec._slice(GEN, 96, 163)).replace("44100", str(SI.SR))
    src = re.sub(r"^(\s*)print (.+)$", r"\1print(\2)", src, flags=re.M)
    exec(compile("\n" * 95 + src, GEN, "exec"), ns)
    err = None
    try:
        ns["__call__"](me, np.array(c))
    except Exception as e:   # what ends the generator's worker; GetOutOfLoop is caught inside
        err = e
    for n in notes:
        del n.getAudio
    return log, np.asarray(seglen, dtype=np.int64), err


def files_of(log):
    """The log as [(chunk, stem, audio, melody_g, melody_e)]."""
    out = []
    for k in range(0, len(log), 3):
        (a, path, audio), (b, _, g), (c, _, e) = log[k:k + 3]
        assert (a, b, c) == ('m', '__g_', '__e_'), (a, b, c)
        assert path.endswith('.data')
        stem = os.path.relpath(path[:-len('.data')], 'FEATURES')
        out.append((int(stem.rsplit('_', 1)[1]), stem, audio, g, e))
    return out


def notes_of(g, seglen, size):
    """Per track the (b, -1, len) of the notes the generator placed, from melody_g and the recorded segment lengths."""
    tracks, k = [], 0
    for i in range(g.shape[0]):
        t = []
        for m in range(g.shape[1]):
            if g[i, m, 2] > 0:
                b = int(np.floor(g[i, m, 0] * SI.HOP))
                t.append((b, -1, int(seglen[k]), min(int(seglen[k]), max(size - b, 0))))
                k += 1
        tracks.append(t)
    assert k == len(seglen)
    return tracks


def main():
    out = {}
    tmp = tempfile.mkdtemp()
    rwc_path = R.write_rwc_tree(os.path.join(tmp, "rwc"))
    db = SI.write_pieces(os.path.join(tmp, "db"))
    util = G.util_ns()
    rwc = G.rwc_ns(util)
    instruments = [rwc["Instrument"](rwc_path, i, list(R.STYLES), list(R.CASES), list(R.DYNAMICS)) for i in R.INSTRUMENT_IDS]
    # --- the combinations
    out["combos_default"] = engine_combos(SI.SHIFTS, ['F', 'M', 'P'], ['NO'], [1, 2, 3], 400, 5)
    out["combos_few_shifts"] = engine_combos([0., 0.2], ['F'], ['NO'], [1], 400, 0)
    out["combos_few_dynamics"] = engine_combos([0.], ['F', 'M'], ['NO'], [1], 10, 3)
    out["combos_single"] = engine_combos([0.], ['F'], ['NO'], [2], 400, 0)
    assert out["combos_default"].shape == (400, 4, 4)
    # --- the renders
    seen = dict(unequal=False, gt=False, overwrite=False, cut=False, past=False)
    for k, (piece, style, ci, chnk) in enumerate(SI.RENDERS):
        c = R.COMBOS[ci]
        log, seglen, err = call(util, instruments, db, piece, style, c)
        assert err is None, err
        files = files_of(log)
        assert [f[0] for f in files] == [0, 1, 2]
        # the segments of the chunk: the recorded lengths are in chunk order
        per_chunk = [int(np.count_nonzero(f[3][:, :, 2] > 0)) for f in files]
        first = sum(per_chunk[:chnk])
        _, stem, audio, g, e = files[chnk]
        seg = seglen[first:first + per_chunk[chnk]]
        out["audio_%d" % k], out["melody_g_%d" % k], out["melody_e_%d" % k] = audio, g, e
        out["stem_%d" % k], out["seglen_%d" % k] = SI.stem_array(stem), seg
        size = audio.shape[0]
        tracks = notes_of(g, seg, size)
        has = dict(unequal=len(set(c[:, 0])) > 1, gt=style == 'gt',
                   overwrite=SI.overwrites([[(b, o, ln) for b, o, _, ln in t if ln > 0] for t in tracks]),
                   cut=any(0 <= b < size and sl > size - b for t in tracks for b, _, sl, _ in t),
                   past=any(b >= size for t in tracks for b, _, _, _ in t))
        for name, v in has.items():
            seen[name] = seen[name] or v
        out["cases_%d" % k] = np.asarray([has[n] for n in sorted(has)], dtype=np.bool_)
        print("render", k, piece, style, audio.shape, g.shape, has)
    assert all(seen.values()), seen
    # the pairs the tests name explicitly
    assert out["cases_0"][sorted(seen).index('unequal')] and out["cases_0"][sorted(seen).index('cut')]
    assert out["cases_1"][sorted(seen).index('gt')] and out["cases_1"][sorted(seen).index('overwrite')]
    assert out["cases_4"][sorted(seen).index('past')]
    # --- where the reference writes no file
    for piece in SI.WRITTEN:
        rows = []
        for ci in SI.WRITTEN_COMBOS:
            log, _, err = call(util, instruments, db, piece, 'original', R.COMBOS[ci])
            rows += [(ci, f[0]) for f in files_of(log[:3 * (len(log) // 3)])]
            print("written", piece, ci, [f[0] for f in files_of(log[:3 * (len(log) // 3)])], type(err).__name__, err)
        out["written_" + piece] = np.asarray(rows, dtype=np.int64).reshape(-1, 2)
    path = os.path.join(HERE, "score_render_si.npz")
    np.savez_compressed(path, **out)
    print("wrote score_render_si.npz, %d bytes" % os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()

"""Writes tests/golden/score_render.npz from the reference's own source.  CPU only; needs the reference tree
(DCS_REFERENCE_ROOT).

    python tests/golden/make_golden_score_render.py

Executed as written on the seeded inputs of tests/score_render_ref.py (a tiny RWC tree and score files in a temporary
directory, sample rate 1000 Hz), with stand-ins only for Python-2 names (``xrange``, ``filter`` returning a list, ``print``
statements rewritten as calls), for file access (a sorted ``os.listdir``; ``genfromtxt`` yielding ``str`` names, as
oracle/ref_exec.py does) and for ``tt`` (it holds the frame and hop sizes and records what ``compute_transform`` is given):

* rwc.py:26-188, ``Instrument`` and ``Note``, on the tree: per instrument the notes it lists (``inst_<id>`` = note number,
  index of the dynamics, player, length of ``getAudio(0)``), and for the instrument whose notes begin with silence
  ``Note.getAudio`` (:154-188) on fresh notes with ``max_duration`` 0 and 3.5 s (``trim_whole_<i>``, ``trim_long_<i>``, the
  start it leaves behind in ``trim_start``);
* ``util.getMidi`` (util.py:331-419) on the four scores for the three 2 s chunks and shifts 0, 0.1 and 0.2
  (``midi_<source>_<chunk>_<shift index>`` = begins, ends, note numbers) and ``util.getMidiLength`` (:517-524);
* ``Engine.__init__`` (examples/bach10/compute_features_bach10rwc.py:59-87) with ``np.random`` = ``RandomState(seed)`` for
  the default setting (27 tuples, 400 of 421 200 permutations: ``combos_default``) and for the ``len(cc) < 4`` branches
  (``combos_few_shifts``, ``combos_few_dynamics``, ``combos_single``);
* the render lines :112-139 for four (combination, chunk) pairs: ``audio_<k> [size, 5]`` and the segment length of every
  note (``seglen_<k>``); for two of them the blocks of oracle/stft_np.compute_file at frame / hop (256, 64) and (1024,
  512) (``block_<k>``);
* examples/bach10/compute_features_bach10sibelius.py:67-79 (``sib_combos``) and :98-123 on four seeded sources for two of
  the combinations (``sib_audio_<k>``), for one of them its block at (4096, 512) (``sib_block_<k>``).
"""
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
for p in (ROOT, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import score_render_ref as R  # noqa: E402
from deepconvsep_amd.separation import blackmanharris  # noqa: E402
from oracle import ref_exec, stft_np  # noqa: E402

RWC = "examples/bach10/compute_features_bach10rwc.py"
SIB = "examples/bach10/compute_features_bach10sibelius.py"


def _run(relpath, first, last, ns):
    src = textwrap.dedent(ref_exec._slice(relpath, first, last))
    src = re.sub(r"^(\s*)print (.+)$", r"\1print(\2)", src, flags=re.M)
    exec(compile("\n" * (first - 1) + src, relpath, "exec"), ns)
    return ns


def _os():
    fake = types.SimpleNamespace(path=os.path, listdir=lambda d: sorted(os.listdir(d)))
    return fake


def util_ns():
    import scipy.io.wavfile  # noqa: F401
    import scipy
    ns = ref_exec.score()
    ns.update(scipy=scipy, os=_os())
    _run("util.py", 47, 54, ns)
    _run("util.py", 331, 419, ns)
    _run("util.py", 517, 524, ns)
    return ns


def rwc_ns(util):
    from scipy import io
    ns = dict(np=np, os=_os(), io=io, util=types.SimpleNamespace(readAudioScipy=util["readAudioScipy"]))
    return _run("rwc.py", 26, 188, ns)


def engine_combos(time_shifts, dynamics, styles, cases, sample_size, seed):
    me = types.SimpleNamespace(allowed_dynamics=dynamics, allowed_styles=styles, allowed_case=cases,
                               sources=['bassoon', 'clarinet', 'saxophone', 'violin'])
    fake_np = types.SimpleNamespace(array=np.array, random=np.random.RandomState(seed))
    ns = dict(np=fake_np, it=itertools, xrange=range, self=me, time_shifts=list(time_shifts), sample_size=sample_size)
    _run(RWC, 59, 87, ns)
    return np.asarray(me.combo, dtype=np.float64)


class GetOutOfLoop(Exception):
    pass


def render(util, instruments, db, c, chnk):
    """:112-139 for the combination ``c`` and chunk ``chnk`` of the piece; every getAudio call is recorded."""
    seglen = []

    def recorded(plain):
        def getAudio(max_duration=0):
            a = plain(max_duration)
            seglen.append(len(a))
            return a
        return getAudio
    notes = [n for ins in instruments for n in ins.notes]
    for n in notes:
        n.getAudio = recorded(n.getAudio)
    me = types.SimpleNamespace(sources=list(R.SOURCES), sources_midi=list(R.SOURCES), sampleRate=R.SR, style_midi=['_original'],
                               instruments=instruments, allowed_dynamics=list(R.DYNAMICS), allowed_styles=list(R.STYLES))
    tt = types.SimpleNamespace(hopSize=64, frameSize=256)
    ns = dict(np=np, os=os, util=types.SimpleNamespace(getMidi=util["getMidi"]), self=me, tt=tt, c=np.array(c), db=db,
              f=R.PIECE, s=0, chunk_size=R.CHUNK, chunk_start=R.CHUNK * chnk, chunk_end=R.CHUNK * (chnk + 1),
              GetOutOfLoop=GetOutOfLoop)
    # the script's sample rate is the constant 44100 (:47, :117); here it is the tree's
    src = textwrap.dedent(ref_exec._slice(RWC, 112, 139)).replace("44100", str(R.SR))
    src = re.sub(r"^(\s*)print (.+)$", r"\1print(\2)", src, flags=re.M)
    exec(compile("\n" * 111 + src, RWC, "exec"), ns)
    for n in notes:
        del n.getAudio
    return np.array(ns["audio"], dtype=np.float64), np.asarray(seglen)


def sibelius(util, combo):
    """:98-123 for one combination on the seeded sources (the wav read of :93 is the stand-in)."""
    src = R.sibelius_sources()
    ns = dict(np=np, c=np.array(combo), sources=list(R.SOURCES), sampleRate=R.SR, blackmanharris=blackmanharris,
              transformFFT=lambda **kw: types.SimpleNamespace(hopSize=kw["hopSize"]))
    for i in range(4):
        ns.update(i=i, sounds=src[i].copy())
        _run(SIB, 98, 123, ns)
    return np.array(ns["audio"], dtype=np.float64)


def block(audio, frame, hop):
    win = blackmanharris(frame)
    return np.stack([stft_np.compute_file(audio[:, j], frameSize=frame, hopSize=hop, window=win) for j in range(audio.shape[1])])


def main():
    out = {}
    tmp = tempfile.mkdtemp()
    rwc_path = R.write_rwc_tree(os.path.join(tmp, "rwc"))
    db = os.path.join(tmp, "db")
    piece = R.write_scores(db)
    util = util_ns()
    rwc = rwc_ns(util)
    # --- the tree
    instruments = []
    for instid in R.INSTRUMENT_IDS:
        ins = rwc["Instrument"](rwc_path, instid, list(R.STYLES), list(R.CASES), list(R.DYNAMICS))
        instruments.append(ins)
        out["inst_%d" % instid] = np.asarray([[n.nr, R.DYNAMICS.index(n.dynamics), c, len(n.getAudio(0))]
                                              for n, c in zip(ins.notes, ins.notes_c)], dtype=np.int64)
        assert all(n.style == 'NO' for n in ins.notes)
    # --- the onset trim
    starts = []
    for k in range(len(R.TRIM_LEADS)):
        a = rwc["Instrument"](rwc_path, R.TRIM_ID, list(R.STYLES), [1], ['F']).notes[k]
        out["trim_whole_%d" % k] = np.array(a.getAudio(0), dtype=np.float64)
        b = rwc["Instrument"](rwc_path, R.TRIM_ID, list(R.STYLES), [1], ['F']).notes[k]
        out["trim_long_%d" % k] = np.array(b.getAudio(R.TRIM_LONG), dtype=np.float64)
        assert a.noteStart == b.noteStart
        starts.append(a.noteStart)
    out["trim_start"] = np.asarray(starts)
    # --- getMidi
    shifts = (0., 0.1, 0.2)
    nframes = int(np.ceil(R.CHUNK * R.SR / np.double(64))) + 2
    for s in R.SOURCES:
        out["midi_length_" + s] = np.asarray(util["getMidiLength"](s + "_g_original", piece), dtype=np.float64)
        for chnk in range(3):
            for j, sh in enumerate(shifts):
                _, b, e, notes = util["getMidi"](s + "_g_original", piece, R.CHUNK * chnk, R.CHUNK * (chnk + 1), R.SR, 64, 256,
                                                 sh, sh, nframes, 1)
                out["midi_%s_%d_%d" % (s, chnk, j)] = np.asarray([b, e, notes], dtype=np.float64)
    # --- the combinations
    out["combos_default"] = engine_combos(shifts, ['F', 'M', 'P'], ['NO'], [1, 2, 3], 400, 5)
    out["combos_few_shifts"] = engine_combos([0., 0.2], ['F'], ['NO'], [1], 400, 0)
    out["combos_few_dynamics"] = engine_combos([0.], ['F', 'M'], ['NO'], [1], 10, 3)
    out["combos_single"] = engine_combos([0.], ['F'], ['NO'], [2], 400, 0)
    assert out["combos_default"].shape == (400, 4, 4), out["combos_default"].shape
    # --- the render
    for k, (ci, chnk, frame, hop) in enumerate(R.RENDERS):
        audio, seglen = render(util, instruments, db, R.COMBOS[ci], chnk)
        out["audio_%d" % k], out["seglen_%d" % k] = audio, seglen
        if frame:
            out["block_%d" % k] = block(audio, frame, hop)
        print("render", k, audio.shape, "notes", len(seglen))
    # --- Sibelius
    ns = dict(np=np, it=itertools, xrange=range, sources=list(R.SOURCES), time_shifts=list(R.SIB_SHIFTS),
              intensity_shifts=list(R.SIB_GAINS))
    _run(SIB, 67, 79, ns)
    out["sib_combos"] = np.asarray([np.asarray(c, dtype=np.float64) for c in ns["combo"]])
    for k, ci in enumerate(R.SIB_PICK):
        audio = sibelius(util, out["sib_combos"][ci])
        out["sib_audio_%d" % k] = audio
        if k == R.SIB_BLOCK:
            out["sib_block_%d" % k] = block(audio, 4096, 512)
        print("sibelius", k, audio.shape)
    path = os.path.join(HERE, "score_render.npz")
    np.savez_compressed(path, **out)
    print("wrote score_render.npz, %d bytes" % os.path.getsize(path))
    assert os.path.getsize(path) < 1 << 20


if __name__ == "__main__":
    main()

"""Writes tests/golden/augment_cs.npz from the reference's own source.  CPU only; needs the reference tree
(DCS_REFERENCE_ROOT).

    python tests/golden/make_golden_augment.py

Executed as written, with stand-ins for ``xrange``, ``it``, ``os`` and a ``tt`` that records what ``compute_transform`` is
given:

* ``util.circular_shift`` (util.py:62-81) on one signal for shifts 0, +-0.2 s, +-0.07 s and +-100 s, with ``min_size`` below
  and above the signal's length (``shift_<i>``; the shifts in ``shift_cs``, the sizes in ``shift_sizes``);
* the combination loop of examples/hiphopss/augmentations/compute_features_cs_aug.py:52-67 (``combos`` [14, 4, 2]) and,
  with one time shift and one intensity, its fallback (``combos_fallback``);
* the activation matrix of compute_features_instr_aug.py:49-53 (``activation``);
* the render and chunk lines of the cs script (:92, :98, :116-147) on four seeded sources for variant 5 of the 14
  (``a_*``) and -- size given, :98 skipped -- for the shifts (-0.2, 0.07, 0, 100) s (``b_*``): the rendered signals
  ``*_rendered [5, size]`` and per chunk the columns handed to compute_transform, transformed by oracle/stft_np.compute_file
  (pinned to the reference's stft_norm) into ``*_block_<i> [5, T, F]`` float64.

The sample rate is 25 Hz, so that the script's own ``30 * sampleRate`` is a chunk of 750 samples and 0.2 s is 5 samples
(odd); frame / hop are (256, 64) for ``a`` and (1024, 512) for ``b``.  Sources are ``synth_audio(L, seed) * 0.25``: the
mixture stays in the amplitude range the STFT bounds of tests/test_gpu_parity.py were established for.
"""
import itertools
import os
import sys
import textwrap
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from deepconvsep_amd.separation import blackmanharris  # noqa: E402
from deepconvsep_amd.synth import synth_audio  # noqa: E402
from oracle import ref_exec, stft_np  # noqa: E402

CS = "examples/hiphopss/augmentations/compute_features_cs_aug.py"
INSTR = "examples/hiphopss/augmentations/compute_features_instr_aug.py"
SR = 25
LENGTHS = (("vocals", 2000), ("bass", 2300), ("drums", 1200), ("other", 1700))     # longer and shorter than the rendered size
SHIFTS = (0., 0.2, -0.2, 0.07, -0.07, 100., -100.)
SIZES = (1500, 2600)


def _run(relpath, first, last, ns):
    exec(compile("\n" * (first - 1) + textwrap.dedent(ref_exec._slice(relpath, first, last)), relpath, "exec"), ns)
    return ns


def circular_shift():
    return _run("util.py", 62, 81, dict(np=np))["circular_shift"]


def combinations(time_shifts, intensity_shifts):
    ns = dict(np=np, it=itertools, xrange=range, sources=['vocals', 'bass', 'drums', 'other'])
    # :52-53 set the two lists; they are the parameters here
    ns.update(time_shifts=list(time_shifts), intensity_shifts=list(intensity_shifts))
    _run(CS, 54, 67, ns)
    return np.asarray([np.asarray(c, dtype=np.float64) for c in ns["combo"]])


def sources():
    return {name: synth_audio(L, seed=11 + i) * 0.25 for i, (name, L) in enumerate(LENGTHS)}


class Recorder(object):
    def __init__(self):
        self.calls = []

    def compute_transform(self, audio, path, phase=False):
        self.calls.append((os.path.basename(path), np.array(audio, dtype=np.float64)))


def render(c, size=None):
    """:92, :98 (unless ``size`` is given) and :116-147 on the seeded sources with the [4, 2] array ``c``."""
    src = sources()
    tt = Recorder()
    fake_os = types.SimpleNamespace(path=types.SimpleNamespace(exists=lambda p: True, join=os.path.join),
                                    makedirs=lambda p: None)
    ns = dict(np=np, os=fake_os, util=types.SimpleNamespace(circular_shift=circular_shift()), tt=tt, c=np.asarray(c),
              sampleRate=SR, feature_path="features", f="song", vocals=src["vocals"].copy(), bass=src["bass"].copy(),
              drums=src["drums"].copy(), others=src["other"].copy())
    _run(CS, 92, 92, ns)
    if size is None:
        _run(CS, 98, 98, ns)
    else:
        ns["size"] = int(size)
    _run(CS, 116, 120, ns)
    rendered = np.stack([ns["mix_raw"], ns["vocals"], ns["bass"], ns["drums"], ns["others"]]).astype(np.float64)
    _run(CS, 122, 147, ns)
    return int(ns["size"]), rendered, [a for _, a in tt.calls]


def blocks(chunks, frame, hop):
    win = blackmanharris(frame)
    return [np.stack([stft_np.compute_file(a[:, j], frameSize=frame, hopSize=hop, window=win) for j in range(5)])
            for a in chunks]


def main():
    out = {}
    x = synth_audio(2000, seed=3) * 0.25
    shift = circular_shift()
    out["shift_x"], out["shift_cs"], out["shift_sizes"] = x, np.asarray(SHIFTS), np.asarray(SIZES)
    for i, (cs, size) in enumerate(itertools.product(SHIFTS, SIZES)):
        out["shift_%d" % i] = np.asarray(shift(x.copy(), min_size=size, cs=cs, sampleRate=SR), dtype=np.float64)
    out["combos"] = combinations([0., 0.2], [1.])
    out["combos_fallback"] = combinations([0.], [1.])
    ns = _run(INSTR, 49, 53, dict(np=np))
    out["activation"] = np.asarray(ns["instrument_activation"], dtype=np.float64)
    for name, L in LENGTHS:
        out["src_" + name] = sources()[name]
    out["sr"] = np.asarray(SR)
    for tag, c, size, frame, hop in (("a", out["combos"][5], None, 256, 64),
                                     ("b", [[-0.2, 1.], [0.07, 1.], [0., 1.], [100., 1.]], 1990, 1024, 512)):
        size, rendered, chunks = render(c, size)
        out[tag + "_c"], out[tag + "_size"], out[tag + "_rendered"] = np.asarray(c, dtype=np.float64), np.asarray(size), rendered
        out[tag + "_frame_hop"] = np.asarray([frame, hop])
        out[tag + "_chunk_lengths"] = np.asarray([len(a) for a in chunks])
        for i, b in enumerate(blocks(chunks, frame, hop)):
            out["%s_block_%d" % (tag, i)] = b
        print(tag, "size", size, "chunks", [len(a) for a in chunks])
    assert out["combos"].shape == (14, 4, 2), out["combos"].shape
    path = os.path.join(HERE, "augment_cs.npz")
    np.savez_compressed(path, **out)
    print("wrote augment_cs.npz, %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()

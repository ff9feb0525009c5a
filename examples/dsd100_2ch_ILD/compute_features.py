#!/usr/bin/env python3
"""Port of the reference's examples/dsd100_2ch_ILD/compute_features_DSD100.py: the stereo training features of DSD100.

    python compute_features.py --db <DSD100 root> [--feature_path <out dir>]

For every song of Mixtures/Dev, in chunks of 30 s plus the rest of the file, two magnitude tensors written by
``transformFFT(1024, 512, hanning).compute_transform``:

    <song>_<i>_in_m_.data   [2, T, 513]   mixture L, R
    <song>_<i>_out_m_.data  [8, T, 513]   vocals L, R, bass L, R, drums L, R, other L, R

(each with its ``.shape``), the pairs ``LargeDatasetMulti`` / ``StereoFeatureWindows`` read.  Default feature path:
<db>/transforms/feature_folder, the reference's.

As shipped the reference script cannot run: it passes ``suffix="in"`` / ``suffix="out"`` to ``compute_transform``, which has
no such keyword, and for a song shorter than 30 s its "rest of file" block reads the loop variable of a loop that never ran.
This port implements the evident intent: the transform's ``suffix`` attribute is set before each call (``saveTensor`` names
the file ``_<suffix>_m_``), and a song shorter than 30 s gives its rest chunk only, as examples/dsd100/compute_features.py
does.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd.separation import read_wav  # noqa: E402
from deepconvsep_amd.transform import transformFFT  # noqa: E402

SOURCES = ("vocals", "bass", "drums", "other")


def stereo(path):
    """[L, 2] float64; a mono file feeds both channels."""
    sr, a = read_wav(path)
    if a.ndim == 1:
        a = a[:, None]
    if a.shape[1] == 1:
        a = np.repeat(a, 2, axis=1)
    return sr, a[:, :2]


def chunk_bounds(n, sampleRate):
    """30 s chunks, then the rest of the file (a song under 30 s: the rest alone)."""
    chunk = 30 * sampleRate
    nblocks = int(n / (float(sampleRate) * 30.0))
    return [(i * chunk, (i + 1) * chunk) for i in range(nblocks)] + [(nblocks * chunk, n)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True, help="the dataset path")
    ap.add_argument("--feature_path", help="the path where to save the features (default <db>/transforms/feature_folder)")
    args = ap.parse_args(argv)
    db = args.db
    feature_path = args.feature_path or os.path.join(db, "transforms", "feature_folder")
    assert os.path.isdir(db), "Please input the directory for the DSD100 dataset with --db path_to_DSD100"
    mix_dir, src_dir = os.path.join(db, "Mixtures"), os.path.join(db, "Sources")
    tt = None
    for f in sorted(os.listdir(os.path.join(mix_dir, "Dev"))):
        if f.startswith('.'):
            continue
        sampleRate, mix = stereo(os.path.join(mix_dir, "Dev", f, "mixture.wav"))
        if tt is None:
            tt = transformFFT(frameSize=1024, hopSize=512, sampleRate=sampleRate, window=np.hanning)
        assert sampleRate == 44100, "Sample rate needs to be 44100"
        os.makedirs(feature_path, exist_ok=True)
        bounds = chunk_bounds(len(mix), sampleRate)
        tt.suffix = "in"
        for i, (a, b) in enumerate(bounds):
            tt.compute_transform(np.array(mix[a:b]), os.path.join(feature_path, f + "_" + str(i) + '.data'), phase=False)
        srcs = [stereo(os.path.join(src_dir, "Dev", f, s + ".wav"))[1] for s in SOURCES]
        tt.suffix = "out"
        for i, (a, b) in enumerate(bounds):
            audio = np.zeros((b - a, 8))
            for j, s in enumerate(srcs):
                audio[:, 2 * j:2 * j + 2] = s[a:b]
            tt.compute_transform(audio, os.path.join(feature_path, f + "_" + str(i) + '.data'), phase=False)
        print("features of %s: %d chunks" % (f, len(bounds)))


if __name__ == "__main__":
    main()

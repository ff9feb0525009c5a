#!/usr/bin/env python3
"""Port of the reference's examples/dsd100/compute_features.py: the training features of DSD100 on the MI355X.

    python compute_features.py --db <DSD100 root> [--feature_path <out dir>]

For every song of Mixtures/Dev: the mono mixture and the four mono sources (vocals, bass, drums, other) in chunks of 30 s
plus the rest of the file, each chunk one ``[5, T, 513]`` magnitude tensor written by ``transformFFT(1024, 512,
blackmanharris).compute_transform`` as ``<song>_<i>__m_.data`` / ``.shape`` (compute_features.py:80-112).  A song shorter
than 30 s gives its rest chunk only (the reference's loop variable would be undefined there).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd.separation import blackmanharris, read_wav  # noqa: E402
from deepconvsep_amd.transform import transformFFT  # noqa: E402

SOURCES = ("vocals", "bass", "drums", "other")


def mono(path):
    sr, a = read_wav(path)
    if a.ndim > 1 and a.shape[1] > 1:
        a = (a[:, 0] + a[:, 1]) / 2
    elif a.ndim > 1:
        a = a[:, 0]
    return sr, a


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True, help="the dataset path")
    ap.add_argument("--feature_path", help="the path where to save the features (default <db>/transforms/t1)")
    args = ap.parse_args(argv)
    db = args.db
    feature_path = args.feature_path or os.path.join(db, "transforms", "t1")
    assert os.path.isdir(db), "Please input the directory for the DSD100 dataset with --db path_to_DSD"
    mix_dir, src_dir = os.path.join(db, "Mixtures"), os.path.join(db, "Sources")
    tt = None
    for f in sorted(os.listdir(os.path.join(mix_dir, "Dev"))):
        if f.startswith('.'):
            continue
        sampleRate, mix = mono(os.path.join(mix_dir, "Dev", f, "mixture.wav"))
        srcs = [mono(os.path.join(src_dir, "Dev", f, s + ".wav"))[1] for s in SOURCES]
        if tt is None:
            tt = transformFFT(frameSize=1024, hopSize=512, sampleRate=sampleRate, window=blackmanharris)
        assert sampleRate == 44100, "Sample rate needs to be 44100"
        os.makedirs(feature_path, exist_ok=True)
        chunk = 30 * sampleRate
        nblocks = int(len(mix) / (float(sampleRate) * 30.0))
        bounds = [(i * chunk, (i + 1) * chunk) for i in range(nblocks)] + [(nblocks * chunk, len(mix))]
        for i, (a, b) in enumerate(bounds):
            audio = np.zeros((b - a, 5))
            audio[:, 0] = mix[a:b]
            for j, s in enumerate(srcs):
                audio[:, 1 + j] = s[a:b]
            tt.compute_transform(audio, os.path.join(feature_path, f + "_" + str(i) + '.data'), phase=False)
        print("features of %s: %d chunks" % (f, len(bounds)))


if __name__ == "__main__":
    main()

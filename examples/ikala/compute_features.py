#!/usr/bin/env python3
"""Port of the reference's examples/ikala/compute_features.py: the training features of iKala on the MI355X.

    python compute_features.py --db <iKala root> [--feature_path <out dir>]

For every Wavfile/*.wav (left channel: accompaniment, right channel: voice) one ``[3, T, 513]`` magnitude tensor --
mixture = left + right, voice = right, accompaniment = left -- written by ``transformFFT(1024, 512, blackmanharris)
.compute_transform`` as ``<name>.data`` / ``.shape`` in <feature_path> (default <db>/transforms/t1).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd.separation import blackmanharris, read_wav  # noqa: E402
from deepconvsep_amd.transform import transformFFT  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True, help="the dataset path")
    ap.add_argument("--feature_path", help="the path where to save the features (default <db>/transforms/t1)")
    args = ap.parse_args(argv)
    db = args.db
    assert os.path.isdir(db), "Please input the directory for the iKala dataset with --db path_to_iKala"
    feature_path = args.feature_path or os.path.join(db, "transforms", "t1")
    tt = None
    for f in sorted(os.listdir(os.path.join(db, "Wavfile"))):
        if not f.endswith(".wav"):
            continue
        sampleRate, audioObj = read_wav(os.path.join(db, "Wavfile", f))
        if tt is None:
            tt = transformFFT(frameSize=1024, hopSize=512, sampleRate=sampleRate, window=blackmanharris)
        assert sampleRate == 44100, "Sample rate needs to be 44100"
        audio = np.zeros((audioObj.shape[0], 3))
        audio[:, 0] = audioObj[:, 0] + audioObj[:, 1]   # mixture = voice + accompaniment
        audio[:, 1] = audioObj[:, 1]                    # voice
        audio[:, 2] = audioObj[:, 0]                    # accompaniment
        os.makedirs(feature_path, exist_ok=True)
        tt.compute_transform(audio, os.path.join(feature_path, f.replace('.wav', '.data')), phase=False)
        print("features of %s" % f)


if __name__ == "__main__":
    main()

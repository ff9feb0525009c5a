#!/usr/bin/env python3
"""Port of the reference's examples/bach10/compute_features_bach10.py: the training features of Bach10 on the MI355X.

    python compute_features.py --db <Bach10 Sources dir> [--feature_path <out dir>] [--frame_size 4096]

For every directory <db>/<piece> whose name starts with a digit, the four files <piece>-{bassoon,clarinet,saxphone,violin}.wav
(the dataset's spelling) give one ``[5, T, frame_size / 2 + 1]`` magnitude tensor -- the mixture (their sum), then the four
sources -- written by ``transformFFT(frame_size, 512, 44100, blackmanharris).compute_transform`` as ``<piece>.data`` /
``.shape`` in <feature_path> (default <db>/transforms/t3).  --frame_size is not in the reference, which uses 4096.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd.separation import blackmanharris, read_wav  # noqa: E402
from deepconvsep_amd.transform import transformFFT  # noqa: E402

SOURCES = ['bassoon', 'clarinet', 'saxphone', 'violin']


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True, help="the Bach10 dataset path (its Sources directory)")
    ap.add_argument("--feature_path", help="the path where to save the features (default <db>/transforms/t3)")
    ap.add_argument("--frame_size", type=int, default=4096)
    args = ap.parse_args(argv)
    db = args.db
    assert os.path.isdir(db), "Please input the directory for the Bach10 dataset with --db path_to_Bach10"
    feature_path = args.feature_path or os.path.join(db, "transforms", "t3")
    tt = transformFFT(frameSize=args.frame_size, hopSize=512, sampleRate=44100, window=blackmanharris)
    for f in sorted(os.listdir(db)):
        if not (os.path.isdir(os.path.join(db, f)) and f[0].isdigit()):
            continue
        for i, source in enumerate(SOURCES):
            sampleRate, audioObj = read_wav(os.path.join(db, f, f + '-' + source + '.wav'))
            assert sampleRate == 44100, "Sample rate needs to be 44100"
            if i == 0:
                audio = np.zeros((audioObj.shape[0], len(SOURCES) + 1))
            audio[:, 0] = audio[:, 0] + audioObj    # mixture = the sum of the four
            audio[:, i + 1] = audioObj
        os.makedirs(feature_path, exist_ok=True)
        tt.compute_transform(audio, os.path.join(feature_path, f + '.data'), phase=False)
        print("features of %s" % f)


if __name__ == "__main__":
    main()

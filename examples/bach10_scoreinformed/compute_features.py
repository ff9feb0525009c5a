#!/usr/bin/env python3
"""Port of the reference's examples/bach10_scoreinformed/compute_features_bach10.py (:56-99): the training features of the
score-informed Bach10 network on the MI355X.

    python compute_features.py --db <Bach10 Sources dir> [--feature_path <out dir>] [--frame_size 4096]

For every directory <db>/<piece> whose name starts with a digit, the four files <piece>-{bassoon,clarinet,saxphone,violin}.wav
(the dataset's spelling) give one ``[5, T, frame_size / 2 + 1]`` magnitude tensor -- the mixture (their sum), then the four
sources -- written by ``transformFFT(frame_size, 512, 44100, blackmanharris).compute_transform`` as ``<piece>__m_.data`` /
``.shape`` in <feature_path> (default <db>/transforms/t3), and the score files {bassoon,clarinet,saxophone,violin}_{g,b}.txt of
the piece give three note tables ``[4, notes, 43]`` next to it (:84-91): ``_g_`` from the ground-truth scores, ``_b_`` from the
aligned scores with a fermata of 0.5 s, ``_e_`` the same with every note 0.2 s early and 0.2 s late -- the one
train_bach10_si.py reads by default (trainCNNrwc.py:658).  --frame_size is not in the reference, which uses 4096.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd.score import expandMidi, getMidiNum  # noqa: E402
from deepconvsep_amd.separation import blackmanharris, read_wav  # noqa: E402
from deepconvsep_amd.transform import transformFFT  # noqa: E402

SOURCES = ['bassoon', 'clarinet', 'saxphone', 'violin']
SOURCES_MIDI = ['bassoon', 'clarinet', 'saxophone', 'violin']
NHARMONICS, INTERVAL, TUNING_FREQ = 20, 50, 440      # :47-49


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
        piece = os.path.join(db, f)
        nelem_g = nelem_b = 1
        for s in SOURCES_MIDI:                                                       # :62-66
            nelem_g = max(getMidiNum(s + '_g', piece, 0, 40.0), nelem_g)
            nelem_b = max(getMidiNum(s + '_b', piece, 0, 40.0), nelem_b)
        melody_g = np.zeros((len(SOURCES), int(nelem_g), 2 * NHARMONICS + 3))
        melody_b = np.zeros((len(SOURCES), int(nelem_b), 2 * NHARMONICS + 3))
        melody_e = np.zeros((len(SOURCES), int(nelem_b), 2 * NHARMONICS + 3))
        for i, source in enumerate(SOURCES):
            sampleRate, audioObj = read_wav(os.path.join(piece, f + '-' + source + '.wav'))
            assert sampleRate == 44100, "Sample rate needs to be 44100"
            if i == 0:
                nframes = int(len(audioObj) / tt.hopSize)
                audio = np.zeros((audioObj.shape[0], len(SOURCES) + 1))
            audio[:, 0] = audio[:, 0] + audioObj    # mixture = the sum of the four
            audio[:, i + 1] = audioObj
            common = (piece, 0, 40.0, INTERVAL, TUNING_FREQ, NHARMONICS, sampleRate, tt.hopSize, tt.frameSize)
            for table, code, spans, fermata in ((melody_g, '_g', (0., 0.), 0.), (melody_b, '_b', (0., 0.), 0.5),
                                                (melody_e, '_b', (0.2, 0.2), 0.5)):   # :84-91
                tmp = expandMidi(SOURCES_MIDI[i] + code, *(common + spans + (nframes,)), fermata=fermata)
                if tmp is None:
                    raise AttributeError("'NoneType' object has no attribute 'shape'")   # what the reference hits (:85)
                table[i, :tmp.shape[0], :] = tmp
        os.makedirs(feature_path, exist_ok=True)
        tt.compute_transform(audio, os.path.join(feature_path, f + '.data'), phase=False)
        tt.saveTensor(melody_g, '_' + tt.suffix + '_g_')
        tt.saveTensor(melody_b, '_' + tt.suffix + '_b_')
        tt.saveTensor(melody_e, '_' + tt.suffix + '_e_')
        print("features of %s" % f)


if __name__ == "__main__":
    main()

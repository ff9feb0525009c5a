#!/usr/bin/env python3
"""Port of the reference's examples/bach10/compute_features_bach10sibelius.py: the training features of the Bach10 Sibelius
renditions, every rendition with its sources shifted against each other, rendered and transformed on the MI355X.

    python compute_features_sibelius.py --db <Bach10 Sibelius dir> [--feature_path <out dir>] [--gt 1]

For every directory <db>/<piece> whose name starts with a digit, the files <piece>_<style>_{bassoon,clarinet,saxophone,
violin}.wav of every style (--gt 1: 'gt', no shifts; --gt 0: 'fast', 'slow' and 'original' with the 78 combinations of the
onset shifts 0, 0.1 and 0.2 s that are not the same for all four) give one ``[5, T, 2049]`` magnitude tensor per
combination -- the mixture, then the four sources -- in <feature_path>/<style>/ (default <db>/transforms/t3_synth_aug_more)
under the reference's file name.  A combination is a virtual file of ``deepconvsep_amd.augment``: the four recordings are
uploaded once per rendition and shifted inside the STFT's loader (csrc/fft_render.hip).  The pieces are taken in sorted order
(the reference's ``os.listdir`` order is arbitrary).
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd import augment, score_render  # noqa: E402
from deepconvsep_amd.separation import blackmanharris, read_wav  # noqa: E402
from deepconvsep_amd.transform import transformFFT  # noqa: E402

SOURCES = ['bassoon', 'clarinet', 'saxophone', 'violin']


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True, help="the Bach10 Sibelius dataset path")
    ap.add_argument("--feature_path", help="the path where to save the features (default <db>/transforms/t3_synth_aug_more)")
    ap.add_argument("--gt", type=int, default=1, help="1: the ground truth aligned rendition, 0: the others")
    a = ap.parse_args(argv)
    db = a.db
    assert os.path.isdir(db), "Please input the directory for the Bach10 Sibelius dataset with --db path_to_Bach10"
    feature_path = a.feature_path or os.path.join(db, 'transforms', 't3_synth_aug_more')
    styles, time_shifts = (['gt'], (0.,)) if a.gt else (['fast', 'slow', 'original'], (0., 0.1, 0.2))
    tt = transformFFT(frameSize=4096, hopSize=512, sampleRate=44100, window=blackmanharris)
    for f in sorted(os.listdir(db)):
        if not (os.path.isdir(os.path.join(db, f)) and f[0].isdigit()):
            continue
        for style in styles:
            signals = {}
            for i, s in enumerate(SOURCES):
                sampleRate, sounds = read_wav(os.path.join(db, f, f + '_' + style + '_' + s + '.wav'))
                assert sampleRate == 44100, "Sample rate needs to be 44100"
                signals[(f, i)] = sounds
            bank = augment.Bank(signals, np.float64)
            vfiles = score_render.sibelius_files([len(signals[(f, i)]) for i in range(len(SOURCES))], time_shifts, (1.,), 44100,
                                                 name=f)
            for vf in vfiles:
                augment.render_features(tt, bank, vf, os.path.join(feature_path, style))
            print("features of %s %s: %d files" % (f, style, len(vfiles)))


if __name__ == "__main__":
    main()

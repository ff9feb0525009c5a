#!/usr/bin/env python3
"""Separate one stereo file with the stereo (ILD) DSD100 network on the MI355X.

    python separate_dsd_ild.py -i <inputfile> -o <outputdir> -m <path_to_model.pkl> [--mwf N] [--resample]

The reference has no separate script for this graph: its only separation code is the "Separating" block of
examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py:291-341, which this runs on one file with that block's hard-coded
hyper-parameters (scale factor 0.3, 30 frames of context, overlap 25, 513 bins, frameSize 1024, hopSize 512, hanning)
and its output names, <outputdir>/<source>.wav, stereo files.  A mono input is fed to both channels.
--mwf N (default 0: the block as it is) puts N iterations of the multichannel Wiener filter between the network and the
inverse transform -- the stage util.py:633-719 left unfinished.  --resample: a file that is not at 44 100 Hz is converted on
the device, separated and written at its own rate instead of being refused.
"""
import getopt
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd.separation import Separator, load_model, read_wav, write_wav  # noqa: E402
from deepconvsep_amd.stereo_training import SOURCES  # noqa: E402

USAGE = 'python separate_dsd_ild.py -i <inputfile> -o <outputdir> -m <path_to_model.pkl> [--mwf N] [--resample]'


def train_auto(filein, outdir, model, scale_factor=0.3, time_context=30, overlap=25, batch_size=32, input_size=513,
               mwf_iters=0, resample=False):
    sampleRate, audio = read_wav(filein)
    if sampleRate != 44100 and not resample:
        print("Sample rate is not 44100")
        return
    if audio.ndim == 1:
        audio = np.repeat(audio[:, None], 2, axis=1)
    sep = Separator('dsd_ild', load_model(model), scale_factor, time_context, overlap, batch_size, input_size, 1024, 512,
                    np.hanning)
    out = sep.separate_stereo(audio[:, :2], mwf_iters=mwf_iters, sample_rate=sampleRate)          # [L, S, 2]
    os.makedirs(outdir, exist_ok=True)
    for i, s in enumerate(SOURCES):
        write_wav(os.path.join(outdir, s + '.wav'), out[:len(audio), i, :], sampleRate)


def main(argv):
    mwf_iters, resample = 0, False
    try:
        opts, args = getopt.getopt(argv, "hi:o:m:", ["ifile=", "odir=", "mfile=", "mwf=", "resample"])
    except getopt.GetoptError:
        print(USAGE)
        sys.exit(2)
    for opt, arg in opts:
        if opt == '-h':
            print(USAGE)
            sys.exit()
        elif opt in ("-i", "--ifile"):
            inputfile = arg
        elif opt in ("-o", "--odir"):
            outdir = arg
        elif opt in ("-m", "--mfile"):
            model = arg
        elif opt == "--mwf":
            mwf_iters = int(arg)
        elif opt == "--resample":
            resample = True
    train_auto(inputfile, outdir, model, 0.3, 30, 25, 32, 513, mwf_iters, resample)


if __name__ == "__main__":
    main(sys.argv[1:])

#!/usr/bin/env python3
"""Drop-in for the reference's examples/bach10/separate_bach10.py, running on MI355X.

    python separate_bach10.py -i <inputfile> -o <outputdir> -m <path_to_model.pkl> [--resample] [--stereo] [--mwf N]

Same options, hard-coded hyper-parameters and output file names as the
reference's main() (examples/bach10/separate_bach10.py); the work is done by
deepconvsep_amd (HIP kernels behind libdcs.so).  The reference's getopt long
option list contains the typo "--mfile" so only -m works there; here --mfile
works as well.
--stereo: a two-channel file gives two-channel stems under the same names (the
network still sees the script's down-mix; its masks are applied to each channel's own
spectrum); --mwf N, with --stereo only, puts N iterations of the multichannel Wiener
filter in front of the inverse transform.
"""
import getopt
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd.separation import (generate_overlapadd, load_model, overlapadd, overlapadd_multi)  # noqa: E402,F401
from deepconvsep_amd.separation import train_auto as _train_auto  # noqa: E402
from deepconvsep_amd.transform import compute_file, compute_inverse  # noqa: E402,F401

USAGE = 'python separate_bach10.py -i <inputfile> -o <outputdir> -m <path_to_model.pkl> [--resample] [--stereo] [--mwf N]'


def train_auto(filein, outdir, model, scale_factor=0.3, time_context=30, overlap=20, batch_size=32, input_size=2049,
               frameSize=None, hopSize=None, resample=False, stereo=False, mwf_iters=0):
    return _train_auto('bach10', filein, outdir, model, scale_factor, time_context, overlap, batch_size, input_size,
                       frameSize, hopSize, resample=resample, stereo=stereo, mwf_iters=mwf_iters)


def main(argv):
    resample, stereo, mwf_iters = False, False, 0
    try:
        opts, args = getopt.getopt(argv, "hi:o:m:", ["ifile=", "odir=", "mfile=", "resample", "stereo", "mwf="])
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
        elif opt == "--resample":
            resample = True
        elif opt == "--stereo":
            stereo = True
        elif opt == "--mwf":
            mwf_iters = int(arg)
    if mwf_iters and not stereo:        # the Wiener filter works on two-channel estimates
        print(USAGE)
        sys.exit(2)
    train_auto(inputfile, outdir, model, 0.3, 30, 25, 32, 2049, 4096, 512, resample=resample, stereo=stereo, mwf_iters=mwf_iters)


if __name__ == "__main__":
    main(sys.argv[1:])

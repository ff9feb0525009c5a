#!/usr/bin/env python3
"""Align the four Bach10 score files to a recording on the MI355X.

    python align_scores.py -i <mix.wav> -s <scoredir> -o <outdir> [--band N] [--resample] [--online]

``<scoredir>`` holds ``bassoon_b.txt, clarinet_b.txt, saxophone_b.txt, violin_b.txt`` (lines ``onset,offset,note``, seconds)
at the score's nominal tempo; the same four files, with onsets and offsets in the recording's time, are written into
``<outdir>``, where ``separate_bach10.py`` finds them when the wav lies there too (or use its ``--align``).  Chroma features of
the recording and of the score, then dynamic time warping, both on the device (``deepconvsep_amd.align``) on frames of 2048
samples every 512.  ``--band N``: only paths within N score frames of the straight line (default: none up to 2^26
cells, an eighth of the longer side beyond).  ``--resample``: accept a file that is not at 44 100 Hz and align it at its own rate.
``--online``: align causally -- the score follower of ``deepconvsep_amd.align.follow_scores``, the one a stream uses
(``separate_stream.py --follow``), instead of the warping path -- with the same outputs, to compare the two.
"""
import getopt
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd.align import align_score_files  # noqa: E402
from deepconvsep_amd.separation import SI_SCORE_FILES  # noqa: E402

USAGE = 'python align_scores.py -i <mix.wav> -s <scoredir> -o <outdir> [--band N] [--resample] [--online]'


def main(argv):
    try:
        opts, args = getopt.getopt(argv, "hi:s:o:", ["ifile=", "sdir=", "odir=", "band=", "resample", "online"])
    except getopt.GetoptError:
        print(USAGE)
        sys.exit(2)
    band, resample, online = 'auto', False, False
    for opt, arg in opts:
        if opt == '-h':
            print(USAGE)
            sys.exit()
        elif opt in ("-i", "--ifile"):
            inputfile = arg
        elif opt in ("-s", "--sdir"):
            scoredir = arg
        elif opt in ("-o", "--odir"):
            outdir = arg
        elif opt == '--band':
            band = int(arg)
        elif opt == '--resample':
            resample = True
        elif opt == '--online':
            online = True
    if online:
        pos, _ = align_score_files(inputfile, scoredir, outdir, SI_SCORE_FILES, resample=resample, online=True)
        print("followed %d score files along %s: %d frames, last position %d" % (len(SI_SCORE_FILES), inputfile, len(pos), pos[-1]))
        return
    path, cost = align_score_files(inputfile, scoredir, outdir, SI_SCORE_FILES, band=band, resample=resample)
    print("aligned %d score files to %s: %d path points, cost %.4f" % (len(SI_SCORE_FILES), inputfile, len(path), cost))


if __name__ == "__main__":
    main(sys.argv[1:])

#!/usr/bin/env python3
"""Port of the reference's examples/bach10_scoreinformed/compute_features_bach10rwc.py: the RWC-sample training data of the
score-informed Bach10 network, every score re-synthesised note by note from RWC instrument samples, assembled and
transformed on the MI355X, with the two note tables the trainer cuts its harmonic masks from.

    python compute_features_rwc.py --db <Bach10 Sibelius dir> --rwc <RWC dir with mat/ and wav/> [--feature_path <out dir>]
                                   [--chunk_size 45] [--sample_size 400] [--original 1] [--seed 0]
                                   [--sample_rate 44100]

For every directory <db>/<piece> whose name starts with a digit and every sampled combination of onset shift, dynamics and
player per instrument, each chunk of --chunk_size seconds of the scores <piece>/<source>_g_original.txt (--original 0:
<source>_g.txt, the ground-truth aligned ones, no shifts, at most 50 combinations) gives three tensors in
<feature_path>/<piece>/<original|gt>/ (default <db>/transforms/t3_rwc) under the reference's file names: ``__m_`` the ``[5,
T, 2049]`` magnitudes -- the mixture, then bassoon, clarinet, saxophone, violin --, ``__g_`` the note table the audio was
rendered from and ``__e_`` the one with the onsets and offsets widened by 0.2 s (``[4, notes, 43]``, util.expandMidi), the
pairs ``ScoreFeatureWindows`` loads.  The note bank is uploaded once; a variant is a note table, and neither its audio nor
anything but the block that is written ever exists (csrc/fft_score_render.hip).

Differences from the reference: the combinations are drawn by RandomState(--seed + index of the piece) (the reference's
draw is unseeded); there is no process pool (--nprocs); where the reference's worker skips a chunk (a note the RWC tree
lacks) or dies (an instrument with fewer than two notes in a chunk, a note that begins past the rendered length) the file is
left out as it is there, and the run goes on with the next combination; see INTEGRATION.md for the note bank's own
differences.  Training needs none of these files: train_bach10_si.py --rwc <RWC dir> --render renders the same windows,
masks included, per batch.
"""
import argparse
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd import score_render  # noqa: E402
from deepconvsep_amd.separation import blackmanharris  # noqa: E402
from deepconvsep_amd.transform import transformFFT  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True, help="the Bach10 Sibelius dataset path")
    ap.add_argument("--rwc", required=True, help="the rwc instrument sound path with mat and wav subfolders")
    ap.add_argument("--feature_path", help="the path where to save the features (default <db>/transforms/t3_rwc)")
    ap.add_argument("--chunk_size", type=float, default=45.0, help="the chunk size to split the midi, in seconds")
    ap.add_argument("--sample_size", type=int, default=400, help="sample this number of combinations of possible cases")
    ap.add_argument("--original", type=int, default=1, help="1: the original score, 0: the ground truth aligned score")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--sample_rate", type=int, default=44100, help="of the RWC recordings (the reference's constant; for tests)")
    a = ap.parse_args(argv)
    assert os.path.isdir(a.db), "Please input the directory for the Bach10 Sibelius dataset with --db path_to_Bach10"
    assert os.path.isdir(a.rwc), "Please input the directory for the RWC instrument sound with --rwc path_to_RWC"
    feature_path = a.feature_path or os.path.join(a.db, 'transforms', 't3_rwc')
    bank = score_render.load_bank(a.rwc)
    tt = transformFFT(frameSize=4096, hopSize=512, sampleRate=a.sample_rate, window=blackmanharris)
    for f, style, sfiles in score_render.si_dataset_files(a.db, bank, a.chunk_size, a.sample_size, bool(a.original), a.seed,
                                                             a.sample_rate, 512, 4096):
        out_dir = os.path.join(feature_path, f, style)
        for sf in sfiles:
            score_render.render_score_informed_features(tt, bank, sf, out_dir)
        print("features of %s: %d files" % (f, len(sfiles)))


if __name__ == "__main__":
    main()

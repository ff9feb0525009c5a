#!/usr/bin/env python3
"""Train the Bach10 separation network on the MI355X: port of the reference's examples/bach10/trainCNNbach10.py.

    python train_bach10.py --db <Bach10 Sources dir> --output <dir> [--dbs <Bach10 Sibelius dir>] [--feature_path P]
                           [--model CNNbach10] [--batch_size 32] [--time_context 30] [--overlap 25] [--nepochs 20]
                           [--scale_factor 0.3] [--scale_factor_test 0.2] [--frame_size 4096] [--load] [--skip]
                           [--skip_sep] [--seed 0] [--windows reference|all]
                           [--rwc <RWC dir> --render [--sample_size 400] [--chunk_size 45] [--original 1]
                                                           [--sample_rate 44100]]

Features come from compute_features.py (``<feature_path>/*.data``, default <db>/transforms/t3).  Per epoch the reference's six
lines are printed and the model is saved as <output>/models/model_<NAME>.pkl (the format separate_bach10.py loads); the
per-epoch loss list is pickled as <output>/models/loss_<NAME>.data.  Then, unless --skip_sep, the mixture of every piece
<db>/<piece> (the sum of its four source files) is separated at --scale_factor_test into
<output>/output/<NAME>/<piece>-<source>.wav, and, when --dbs is given, the Sibelius renditions
<dbs>/<piece>/<piece>_{fast,slow,original}_<source>.wav into <output>/output/<NAME>_original/.

The reference trains this one graph from three scripts -- trainCNNbach10.py, trainCNNrwc.py and trainCNNSibelius.py have the
same build_ca and the same loss and differ only in where their features come from -- so --feature_path pointing at features
made any other way (``[5, T, F]`` .data files: mixture, bassoon, clarinet, saxophone, violin) is the use of the other two.

With --rwc PATH --render (the use of trainCNNrwc.py without its feature files) the windows are those of
compute_features_rwc.py -- the scores of --dbs re-synthesised from the RWC note samples under PATH in --sample_size
combinations per piece, chunks of --chunk_size seconds -- assembled and transformed per batch from the note bank resident on
the device (``ScoreRenderedWindows``, csrc/fft_score_render.hip); no feature file is read or written, and --frame_size sets
the transform.  Without these flags nothing changes.

Differences from the reference: the window order of an epoch is RandomState(seed + epoch).permutation (the reference's
shuffle is unseeded); --scale_factor and --scale_factor_test are floats (the reference's int() of them is a bug); --load,
--skip and --skip_sep are flags (the reference has no way to skip the separation); --dbs is optional and its loop is skipped
without it (the reference asserts the directory exists); --windows all takes every full window instead of the first
getNum(T) ones that LargeDataset fills; --frame_size (the reference's transform is fixed at 4096, 2049 bins, where one model
is 856 MB) sets the STFT frame of the separation and must match the features'.
"""
import argparse
import glob
import os
import pickle
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd import score_render  # noqa: E402
from deepconvsep_amd.separation import Separator, blackmanharris, load_model, read_wav, write_wav  # noqa: E402
from deepconvsep_amd.training import BACH10_COMPONENTS, FeatureWindows, Trainer  # noqa: E402

SOURCES = ['bassoon', 'clarinet', 'saxphone', 'violin']            # the file names of the Bach10 dataset
SOURCES_MIDI = ['bassoon', 'clarinet', 'saxophone', 'violin']      # those of the Sibelius renditions
STYLES = ['fast', 'slow', 'original']


def separate_mixture(sep, files, outfiles):
    """trainCNNbach10.py:263-296: the mixture is the sum of the source files; one output file per source."""
    audio = None
    for filename in files:
        sampleRate, audioObj = read_wav(filename)
        assert sampleRate == 44100, "Sample rate needs to be 44100"
        audio = audioObj.copy() if audio is None else audio + audioObj
    out = sep.separate(audio)
    for i, filename in enumerate(outfiles):
        write_wav(filename, out[i][:len(audio)], sampleRate)


def separate_all(params, db, dbs, pieces, outdir, outdir1, scale_factor, tc, overlap, batch_size, frame_size):
    """trainCNNbach10.py:256-337 with the fused separation path."""
    sep = Separator('bach10', params, scale_factor, tc, overlap, batch_size, frame_size // 2 + 1, frame_size, 512,
                    blackmanharris)
    os.makedirs(outdir, exist_ok=True)
    for f in pieces:
        separate_mixture(sep, [os.path.join(db, f, f + '-' + s + '.wav') for s in SOURCES],
                         [os.path.join(outdir, f + '-' + s + '.wav') for s in SOURCES])
    if dbs is None:
        return
    os.makedirs(outdir1, exist_ok=True)
    for style in STYLES:
        for f in pieces:
            separate_mixture(sep, [os.path.join(dbs, f, f + '_' + style + '_' + s + '.wav') for s in SOURCES_MIDI],
                             [os.path.join(outdir1, f + '_' + style + '_' + s + '.wav') for s in SOURCES_MIDI])


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True, help="the Bach10 dataset path (its Sources directory)")
    ap.add_argument("--dbs", help="the Bach10 Sibelius dataset path")
    ap.add_argument("--output", required=True, help="the path where to save the model and the output")
    ap.add_argument("--feature_path")
    ap.add_argument("--model", default="CNNbach10")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--time_context", type=int, default=30)
    ap.add_argument("--overlap", type=int, default=25)
    ap.add_argument("--nepochs", type=int, default=20)
    ap.add_argument("--scale_factor", type=float, default=0.3)
    ap.add_argument("--scale_factor_test", type=float, default=0.2)
    ap.add_argument("--frame_size", type=int, default=4096)
    ap.add_argument("--load", action="store_true", help="resume from models/model_<model>.pkl")
    ap.add_argument("--skip", action="store_true", help="skip training")
    ap.add_argument("--skip_sep", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--windows", choices=("reference", "all"), default="reference")
    ap.add_argument("--rwc", help="the rwc instrument sound path with mat and wav subfolders (with --render)")
    ap.add_argument("--render", action="store_true", help="train on the scores of --dbs rendered from --rwc, without feature files")
    ap.add_argument("--sample_size", type=int, default=400)
    ap.add_argument("--chunk_size", type=float, default=45)
    ap.add_argument("--original", type=int, default=1)
    ap.add_argument("--sample_rate", type=int, default=44100, help="of the RWC recordings, with --render (for tests)")
    a = ap.parse_args(argv)
    if a.render != (a.rwc is not None):
        ap.error("--rwc PATH and --render go together")
    if a.render and a.dbs is None:
        ap.error("--render takes the scores from --dbs")
    db, output = a.db, a.output
    assert os.path.isdir(db), "Please input the directory for the Bach10 dataset with --db path_to_Bach10"
    assert a.dbs is None or os.path.isdir(a.dbs), \
        "Please input the directory for the Bach10 Sibelius dataset with --dbs path_to_Bach10Sibelius"
    assert os.path.isdir(output), "Please input the output directory --output path_to_output"
    feature_path = a.feature_path or os.path.join(db, 'transforms', 't3')
    pieces = [f for f in sorted(os.listdir(db)) if os.path.isdir(os.path.join(db, f)) and f[0].isdigit()]
    os.makedirs(os.path.join(output, 'models'), exist_ok=True)
    model = os.path.join(output, 'models', "model_" + a.model + ".pkl")
    params = load_model(model) if a.load else None
    F = a.frame_size // 2 + 1
    if not a.skip:
        if a.render:
            assert os.path.isdir(a.rwc), "Please input the directory for the RWC instrument sound with --rwc path_to_RWC"
            bank = score_render.load_bank(a.rwc)
            chunk = int(a.chunk_size) if a.chunk_size == int(a.chunk_size) else a.chunk_size
            sfiles = [sf for _, _, v in score_render.dataset_files(a.dbs, bank, chunk, a.sample_size, bool(a.original), a.seed,
                                                                      a.sample_rate) for sf in v]
            if not sfiles:
                raise SystemExit("no score under %s could be rendered from %s" % (a.dbs, a.rwc))
            data = score_render.ScoreRenderedWindows(bank, sfiles, a.time_context, a.overlap, a.scale_factor, a.windows,
                                                     a.batch_size, a.seed, None, a.frame_size, 512, blackmanharris)
        else:
            paths = sorted(glob.glob(os.path.join(feature_path, "*.data")))
            if not paths:
                raise SystemExit("no .data feature files under %s: run compute_features.py first" % feature_path)
            data = FeatureWindows(paths, a.time_context, a.overlap, a.scale_factor, a.windows, a.batch_size, a.seed)
        if data.iteration_size == 0:
            raise SystemExit("%d windows are fewer than one batch of %d" % (data.total, a.batch_size))
        if data.F != F:
            raise SystemExit("the features have %d bins, --frame_size %d gives %d" % (data.F, a.frame_size, F))
        trainer = Trainer(arch='bach10', params=params, batch_size=a.batch_size, time_context=a.time_context,
                          feat_size=data.F, seed=a.seed)
        losser = []
        for epoch in range(a.nepochs):
            start_time = time.time()
            err = 0.0
            comp = np.zeros(4)
            for inputs, targets in data.batches(epoch):
                err += trainer.step(inputs, targets)                 # train_fn (trainCNNbach10.py:238)
                comp += np.asarray(trainer.losses(inputs, targets))  # train_fn1 (:239)
            n = data.iteration_size
            print("Epoch {} of {} took {:.3f}s".format(epoch + 1, a.nepochs, time.time() - start_time))
            print("  training loss:\t\t{:.6f}".format(err / n))
            for k, name in enumerate(BACH10_COMPONENTS):
                print("  training loss for {}:\t\t{:.6f}".format(name, comp[k] / n))
            losser.append(err / n)
            trainer.save_model(model)
        with open(os.path.join(output, 'models', "loss_" + a.model + ".data"), 'wb') as f:
            pickle.dump(losser, f, protocol=2)
        params = trainer.params()
        trainer.close()
    if not a.skip_sep:
        if params is None:
            raise SystemExit("--skip without --load leaves no model to separate with")
        separate_all(params, db, a.dbs, pieces, os.path.join(output, 'output', a.model),
                     os.path.join(output, 'output', a.model + "_original"), a.scale_factor_test, a.time_context,
                     a.overlap, a.batch_size, a.frame_size)


if __name__ == "__main__":
    main()

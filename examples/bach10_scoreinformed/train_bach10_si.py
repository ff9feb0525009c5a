#!/usr/bin/env python3
"""Train the score-informed Bach10 separation network on the MI355X: port of the reference's
examples/bach10_scoreinformed/trainCNNrwc.py with ``--function build_ca`` (the first half of train_auto and its separation
block, :196-416).

    python train_bach10_si.py --db <Bach10 Sources dir> --output <dir> [--feature_path P] [--model CNNrwc_se1]
                              [--batch_size 32] [--time_context 30] [--overlap 25] [--nepochs 40] [--scale_factor 0.3]
                              [--scale_factor_test 0.2] [--pitch_code e] [--branches 4|1] [--frame_size 4096] [--load]
                              [--skip] [--skip_sep] [--second_pass] [--seed 0] [--windows reference|all]
                              [--function build_ca|build_ca_1x1]
                              [--dbs <Bach10 Sibelius dir> --rwc <RWC dir> --render [--sample_size 400] [--chunk_size 45]
                                                                                    [--original 1] [--sample_rate 44100]]

Features and note tables come from compute_features.py (``<feature_path>/*_m_.data`` with their ``_<pitch_code>_`` tables,
default <db>/transforms/t3).  The network's input is the mixture times the four harmonic masks of the score, cut for every
window on the device (``ScoreFeatureWindows``).  Per epoch the reference's six lines are printed (:333-339) and the model is
saved when the epoch loss improves (:342-344) as <output>/models/model_<NAME>_gt.pkl (:633-639: the ``gt`` style), the format
separate_bach10.py loads; the per-epoch loss list is pickled as <output>/models/loss_<NAME>_gt.data.  Then, unless --skip_sep,
every piece <db>/<piece> is separated as :363-416 do: the mixture is the sum of its four source files, the masks come from
its ``_b`` score files and ``LargeDatasetMask2.filterSpec``, the soft masks are applied to the sum of the input channels
(``Separator('bach10_si', ..., score_normalise='sum', score_mixture='sum')``), --scale_factor_test scales the magnitudes; the
results go to <output>/output/<NAME>_gt/<piece>-<source>.wav.

With --dbs DIR --rwc PATH --render (the reference's own use of this script, trainCNNrwc.py on the data of
compute_features_bach10rwc.py, without its feature files) the windows are those of compute_features_rwc.py -- the scores of
--dbs re-synthesised from the RWC note samples under PATH in --sample_size combinations per piece -- rendered, transformed and
masked per batch on the device (``ScoreInformedRenderedWindows``, csrc/fft_score_render.hip); no feature file is read or
written, --frame_size sets the transform and --pitch_code is e or g.

--branches 1 trains the single-branch 11-array layout of trainCNNrwc_samp.py:195-235 (the same live computation and loss;
the 17-array layout's other three branches are dead weight that no gradient reaches).

--second_pass ports :346-354: after the --nepochs Adadelta epochs, if the last epoch's loss is above the best one the best
model is loaded back into the live trainer (``set_params``), the optimiser becomes ``lasagne.updates.adam`` with its defaults
(``set_optimizer('adam')``, csrc/train_core.hip's adam_kernel) and int(ceil(nepochs / 5)) more epochs run, printed as "Epoch k
of n2", with the same save-on-improvement rule; the loss list and the best loss carry over, and epoch k of the second pass
cuts the windows of ``batches(nepochs + k)``.  It is a property of the loop alone: every --function, --branches and feed takes it.

--function build_ca_1x1 trains the deep graph of trainCNNrwc.py:66-132 (six strided convolutions, a 1x1 convolution and
their InverseLayers; 22 arrays) with the same loss and feeds; as in the reference (:630-639) any other value means build_ca,
and the 1x1 choice appends ``_x`` to the model name before the style suffix: model_<NAME>_x_gt.pkl.  It needs --time_context
>= 19 and --frame_size >= 504; --branches 1 writes its live-only layout.

Differences from the reference: the window order of an epoch is RandomState(seed + epoch).permutation (the reference's shuffle
is unseeded); --scale_factor and --scale_factor_test are floats (the reference's int() of them is a bug); --load, --skip and
--skip_sep are flags; --pitch_code, --branches, --windows and --frame_size are new (the reference's transform is fixed at 4096,
2049 bins; --frame_size must match the features'); the second pass with Adam (:346-354) runs only with --second_pass, and
its reload of the best model is the evident intent of :349-351, which as written raises in Lasagne (set_all_param_values
reads ``learning_rate=0.0001`` as a parameter tag) -- so Adam runs at lasagne.updates.adam's own learning rate 1e-3, as :353
builds it; with --nepochs 0 no second pass runs (the reference fails on ``losser[-1]``), and after the second pass the
reference's loop would reach :349-351 once more, while here the separation uses the network as it stands; the Sibelius loop
of the reference is commented out there (:418-) and absent here; features are read from one flat directory rather than from
<feature_path>/<piece>/gt.
"""
import argparse
import math
import os
import pickle
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd import score_render  # noqa: E402
from deepconvsep_amd.score import melody_table  # noqa: E402
from deepconvsep_amd.score_training import COMPONENTS, ScoreFeatureWindows, ScoreTrainer  # noqa: E402
from deepconvsep_amd.separation import Separator, blackmanharris, load_model, read_wav, write_wav  # noqa: E402

SOURCES = ['bassoon', 'clarinet', 'saxphone', 'violin']            # the file names of the Bach10 dataset (:360)
SOURCES_MIDI = ['bassoon', 'clarinet', 'saxophone', 'violin']      # those of its score files (:361)
NHARMONICS, INTERVAL, TUNING_FREQ = 20, 50, 440                    # :231-233


def separate_all(params, db, pieces, outdir, scale_factor, tc, overlap, batch_size, frame_size):
    """trainCNNrwc.py:363-416 with the fused score-informed separation path."""
    sep = Separator('bach10_si', params, scale_factor, tc, overlap, batch_size, frame_size // 2 + 1, frame_size, 512,
                    blackmanharris, tiler='library', score_normalise='sum', score_mixture='sum')
    os.makedirs(outdir, exist_ok=True)
    for f in pieces:
        audio = None
        for s in SOURCES:
            sampleRate, audioObj = read_wav(os.path.join(db, f, f + '-' + s + '.wav'))
            assert sampleRate == 44100, "Sample rate needs to be 44100"
            audio = audioObj.copy() if audio is None else audio + audioObj
        nframes = int(np.ceil(len(audio) / np.double(512))) + 2                                    # :375
        melody = melody_table([s + '_b' for s in SOURCES_MIDI], os.path.join(db, f), nframes, sampleRate, 512, frame_size,
                              interval=INTERVAL, tuning_freq=TUNING_FREQ, nharmonics=NHARMONICS, beginTime=0, finishTime=40.0,
                              timeSpan_on=0.2, timeSpan_off=0.2, fermata=0.5)                      # :366-382
        out = sep.separate_scoreinformed(audio, melody)
        for i, s in enumerate(SOURCES):
            write_wav(os.path.join(outdir, f + '-' + s + '.wav'), out[i][:len(audio)], sampleRate)


def network_function(value):
    """trainCNNrwc.py:627-631: ``build_ca_1x1`` if asked for by name, ``build_ca`` for anything else."""
    return 'build_ca_1x1' if value == 'build_ca_1x1' else 'build_ca'


def model_name(model, function):
    """trainCNNrwc.py:633-639: the 1x1 graph's models carry ``_x``, then the ``gt`` style suffix."""
    return model + ('_x' if function == 'build_ca_1x1' else '') + '_gt'


def second_pass_epochs(nepochs):
    """trainCNNrwc.py:347: the second pass runs ``int(np.ceil(float(num_epochs) / 5.))`` epochs; none after no first pass
    (the reference would fail on ``losser[-1]``, :349)."""
    return int(math.ceil(nepochs / 5.)) if nepochs > 0 else 0


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True, help="the Bach10 dataset path (its Sources directory)")
    ap.add_argument("--output", required=True, help="the path where to save the model and the output")
    ap.add_argument("--feature_path")
    ap.add_argument("--model", default="CNNrwc_se1")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--time_context", type=int, default=30)
    ap.add_argument("--overlap", type=int, default=25)
    ap.add_argument("--nepochs", type=int, default=40)
    ap.add_argument("--scale_factor", type=float, default=0.3)
    ap.add_argument("--scale_factor_test", type=float, default=0.2)
    ap.add_argument("--pitch_code", default="e", help="which note tables to train from: e (default), b or g")
    ap.add_argument("--branches", type=int, choices=(4, 1), default=4, help="4: the 17-array model; 1: the 11-array one")
    ap.add_argument("--frame_size", type=int, default=4096)
    ap.add_argument("--load", action="store_true", help="resume from the saved model")
    ap.add_argument("--skip", action="store_true", help="skip training")
    ap.add_argument("--skip_sep", action="store_true")
    ap.add_argument("--second_pass", action="store_true", help="then ceil(nepochs / 5) more epochs with Adam (:346-354)")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--windows", choices=("reference", "all"), default="reference")
    ap.add_argument("--dbs", help="the Bach10 Sibelius dataset path (with --render)")
    ap.add_argument("--rwc", help="the rwc instrument sound path with mat and wav subfolders (with --render)")
    ap.add_argument("--render", action="store_true", help="train on the scores of --dbs rendered from --rwc, without feature files")
    ap.add_argument("--sample_size", type=int, default=400)
    ap.add_argument("--chunk_size", type=float, default=45.0)
    ap.add_argument("--original", type=int, default=1)
    ap.add_argument("--sample_rate", type=int, default=44100, help="of the RWC recordings, with --render (for tests)")
    ap.add_argument("--function", default="build_ca", help="build_ca (default) or build_ca_1x1; anything else is build_ca")
    a = ap.parse_args(argv)
    function = network_function(a.function)
    if a.render != (a.rwc is not None):
        ap.error("--rwc PATH and --render go together")
    if a.render and a.dbs is None:
        ap.error("--render takes the scores from --dbs")
    db, output = a.db, a.output
    assert os.path.isdir(db), "Please input the directory for the Bach10 dataset with --db path_to_Bach10"
    assert os.path.isdir(output), "Please input the output directory --output path_to_output"
    feature_path = a.feature_path or os.path.join(db, 'transforms', 't3')
    pieces = [f for f in sorted(os.listdir(db)) if os.path.isdir(os.path.join(db, f)) and f[0].isdigit()]
    name = model_name(a.model, function)
    os.makedirs(os.path.join(output, 'models'), exist_ok=True)
    model = os.path.join(output, 'models', "model_" + name + ".pkl")
    params = load_model(model) if a.load else None
    F = a.frame_size // 2 + 1
    if not a.skip:
        if a.render:
            assert os.path.isdir(a.dbs), \
                "Please input the directory for the Bach10 Sibelius dataset with --dbs path_to_Bach10Sibelius"
            assert os.path.isdir(a.rwc), "Please input the directory for the RWC instrument sound with --rwc path_to_RWC"
            bank = score_render.load_bank(a.rwc)
            sfiles = [sf for _, _, v in score_render.si_dataset_files(a.dbs, bank, a.chunk_size, a.sample_size, bool(a.original),
                                                                         a.seed, a.sample_rate, 512, a.frame_size) for sf in v]
            if not sfiles:
                raise SystemExit("no score under %s could be rendered from %s" % (a.dbs, a.rwc))
            data = score_render.ScoreInformedRenderedWindows(
                bank, sfiles, a.pitch_code, time_context=a.time_context, overlap=a.overlap, mult_factor=a.scale_factor,
                windows=a.windows, batch_size=a.batch_size, seed=a.seed, frameSize=a.frame_size, hopSize=512)
        else:
            assert os.path.isdir(feature_path), \
                "Please input the directory where you stored the training features --feature_path path_to_features"
            data = ScoreFeatureWindows([feature_path], a.pitch_code, a.time_context, a.overlap, a.scale_factor, a.windows,
                                       a.batch_size, a.seed)
            if not data.pairs:
                raise SystemExit("no _m_.data feature files under %s: run compute_features.py first" % feature_path)
        if data.iteration_size == 0:
            raise SystemExit("%d windows are fewer than one batch of %d" % (data.total, a.batch_size))
        if data.F != F:
            raise SystemExit("the features have %d bins, --frame_size %d gives %d" % (data.F, a.frame_size, F))
        narrays = 22 if function == 'build_ca_1x1' else (17 if a.branches == 4 else 11)
        if params is not None and len(params) != narrays:
            raise SystemExit("%s holds %d arrays, --function %s --branches %d trains %d" % (model, len(params), function,
                                                                                            a.branches, narrays))
        trainer = ScoreTrainer(params=params, branches=a.branches, batch_size=a.batch_size, time_context=a.time_context,
                               feat_size=data.F, seed=a.seed, function=function)
        losser = []
        min_loss = [1e14]                                                                          # :288

        def run_epochs(count, first):
            """``count`` epochs of :295-344; epoch k cuts the windows of ``data.batches(first + k)``."""
            for epoch in range(count):
                start_time = time.time()
                err = 0.0
                comp = np.zeros(4)
                for inputs, targets in data.batches(first + epoch):
                    err += trainer.step(inputs, targets)                 # train_fn (:325)
                    comp += np.asarray(trainer.losses(inputs, targets))  # train_fn1 (:326)
                n = data.iteration_size
                print("Epoch {} of {} took {:.3f}s".format(epoch + 1, count, time.time() - start_time))
                print("  training loss:\t\t{:.6f}".format(err / n))
                for k, source in enumerate(COMPONENTS):
                    print("  training loss for {}:\t\t{:.6f}".format(source, comp[k] / n))
                losser.append(err / n)
                if err / n < min_loss[0]:                                                          # :342-344
                    min_loss[0] = err / n
                    trainer.save_model(model)

        run_epochs(a.nepochs, 0)
        n2 = second_pass_epochs(a.nepochs) if a.second_pass else 0
        if n2:                                                                                     # :346-354
            if losser[-1] > min_loss[0]:
                trainer.set_params(load_model(model))
            trainer.set_optimizer('adam')
            run_epochs(n2, a.nepochs)
        with open(os.path.join(output, 'models', "loss_" + name + ".data"), 'wb') as f:
            pickle.dump(losser, f, protocol=2)
        params = trainer.params()                                    # the separation uses the network as it stands (:357)
        trainer.close()
    if not a.skip_sep:
        if params is None:
            raise SystemExit("--skip without --load leaves no model to separate with")
        separate_all(params, db, pieces, os.path.join(output, 'output', name), a.scale_factor_test, a.time_context,
                     a.overlap, a.batch_size, a.frame_size)


if __name__ == "__main__":
    main()

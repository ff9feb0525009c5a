#!/usr/bin/env python3
"""Train the stereo (ILD) DSD100 network in three stages on the MI355X: port of train_auto and __main__ of the reference's
examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100_3stages.py.

    python train_dsd_ild_3stages.py --db <DSD100 root> --output <dir> [--feature_path F] [--model NAME] [--batch_size 32]
                                    [--time_context 30] [--overlap 25] [--nepochs_mse 30] [--nepochs_ILD 10]
                                    [--scale_factor 0.3] [--scale_factor_test 0.3] [--load] [--skip_train_mse]
                                    [--skip_train_ILD] [--binaural] [--skip_sep] [--seed 0] [--windows reference|all]
                                    [--mwf N]

Features come from compute_features.py (``<feature_path>/*_in_m_.data`` / ``*_out_m_.data``, default
<db>/transforms/feature_folder).  Without --load the model's name is <NAME>_mseEp=<nepochs_mse or 0>_ILDEp=<nepochs_ILD or 0>
(0 for a skipped stage, :538-541), with --load it is <NAME> and training starts from <output>/models/<name>.pkl (:169-171).

Stage 1 (mse, unless --skip_train_mse) runs --nepochs_mse epochs of train_fn_mse + train_fn1 and saves
<output>/models/<name>_noILD.pkl after each (:236-260).  Stage 2 (ILD, unless --skip_train_ILD) loads the _noILD parameters
back when stage 1 ran, rebuilds ``adadelta`` -- fresh accumulators, ``set_optimizer('adadelta')`` -- and runs --nepochs_ILD
epochs of train_fn_ILD, saving <name>_ILD.pkl after each (:264-292).  Stage 3 (mse again, unless --skip_train_mse) loads the
_ILD parameters and runs --nepochs_mse more epochs of train_fn_mse, saving <name>_ILD_extra_mse.pkl after each (:295-324).
The reference builds ``adadelta`` anew at :301 but never compiles it into a function: stage 3 calls the train_fn_mse of :204,
whose updates hold the accumulators stage 1 ended with.  So does this script: one trainer runs all three stages, its
``optimizer_state()`` is kept on the host across stage 2 and put back (``load_optimizer_state``) before stage 3.
The loss list (stages 1 and 2) is pickled as <output>/models/loss_<name>.data.  Then, unless --skip_sep, mixture.wav
(--binaural: binaural.wav, :543-546) of every song under Mixtures/{Dev,Test} is separated with the network as it stands into
<output>/output/<name>/Sources/<sub>/<song>/<source>.wav, stereo files; --mwf N (default 0: the reference's block) runs N
iterations of the multichannel Wiener filter between the network and the inverse transform.

Differences from the reference: the two normal draws of the loss are replaced before every step from a device generator
seeded with --seed (Theano's RandomStreams(128) stream is not reproduced); the window order of an epoch is RandomState(seed
+ epoch).permutation with the epochs counted through the stages (the reference's shuffle is unseeded); the scale factors
are floats (the reference's int() of them is a bug) and the skip / load options are flags; --windows all takes every full
window instead of the first getNum(T) ones that LargeDatasetMulti fills; the loss list ends with stage 2 (the reference
also appends stage 3's epochs, :324); a stage of 0 epochs still writes its file, where the reference then meets an
undefined name (model_noILD :266, model_ILD :298); --skip_train_ILD without --skip_train_mse meets the undefined model_ILD
at :298 in the reference, and here stage 3 starts from <name>_ILD.pkl if that file exists and stops with a message if not;
with both stages skipped and no --load the reference separates with the untrained network, here that is an error.
"""
import argparse
import os
import pickle
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from deepconvsep_amd.separation import load_model  # noqa: E402
from deepconvsep_amd.stereo_training import RAND_STD, SOURCES, StereoFeatureWindows, StereoTrainer  # noqa: E402
from train_dsd_ild import separate_all  # noqa: E402


def model_name(model, nepochs_mse, nepochs_ILD, skip_train_mse, skip_train_ILD, load):
    """trainCNN_ILD_DSD100_3stages.py:538-541: the epochs each kind of stage runs are part of the name unless --load."""
    if load:
        return model
    return model + '_mseEp=' + str(0 if skip_train_mse else nepochs_mse) + '_ILDEp=' + str(0 if skip_train_ILD else nepochs_ILD)


def stage_files(output, name):
    """The model train_auto is given (:570) and the three files its stages write (:257, :289, :321)."""
    model = os.path.join(output, 'models', name + '.pkl')
    return model, model[:-4] + '_noILD.pkl', model[:-4] + '_ILD.pkl', model[:-4] + '_ILD_extra_mse.pkl'


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True)
    ap.add_argument("--output", required=True, help="the path where to save the model and the output")
    ap.add_argument("--feature_path")
    ap.add_argument("--model", default="model_name")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--time_context", type=int, default=30)
    ap.add_argument("--overlap", type=int, default=25)
    ap.add_argument("--nepochs_mse", type=int, default=30, help="epochs of each of the two MSE stages")
    ap.add_argument("--nepochs_ILD", type=int, default=10, help="epochs of the ILD stage")
    ap.add_argument("--scale_factor", type=float, default=0.3)
    ap.add_argument("--scale_factor_test", type=float, default=0.3)
    ap.add_argument("--load", action="store_true", help="start from <output>/models/<model>.pkl")
    ap.add_argument("--skip_train_mse", action="store_true", help="skip the two MSE stages")
    ap.add_argument("--skip_train_ILD", action="store_true", help="skip the ILD stage")
    ap.add_argument("--binaural", action="store_true", help="separate binaural.wav instead of mixture.wav")
    ap.add_argument("--skip_sep", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--windows", choices=("reference", "all"), default="reference")
    ap.add_argument("--mwf", type=int, default=0, help="iterations of the multichannel Wiener filter when separating")
    a = ap.parse_args(argv)
    db, output = a.db, a.output
    assert os.path.isdir(db), "Please input the directory for the DSD100 dataset with --db path_to_DSD100"
    assert os.path.isdir(output), "Please input the output directory --output path_to_output"
    os.makedirs(os.path.join(output, 'models'), exist_ok=True)
    name = model_name(a.model, a.nepochs_mse, a.nepochs_ILD, a.skip_train_mse, a.skip_train_ILD, a.load)
    model, model_noILD, model_ILD, model_ILD_extra_mse = stage_files(output, name)
    params = load_model(model) if a.load else None
    if a.skip_train_mse and a.skip_train_ILD:
        if params is None and not a.skip_sep:
            raise SystemExit("--skip_train_mse --skip_train_ILD without --load leaves no model to separate with")
    else:
        import torch
        if not a.skip_train_mse and a.skip_train_ILD and not os.path.isfile(model_ILD):
            raise SystemExit("--skip_train_ILD: the second MSE stage starts from %s, which does not exist" % model_ILD)
        feature_path = a.feature_path or os.path.join(db, 'transforms', 'feature_folder')
        assert os.path.isdir(feature_path), "Please input the directory where you stored the training features " \
            "--feature_path path_to_features"
        data = StereoFeatureWindows([feature_path], a.time_context, a.overlap, a.scale_factor, a.scale_factor, a.windows,
                                    a.batch_size, a.seed)
        if not data.pairs:
            raise SystemExit("no *_in_m_.data / *_out_m_.data pairs under %s: run compute_features.py first" % feature_path)
        if data.iteration_size == 0:
            raise SystemExit("%d windows are fewer than one batch of %d" % (data.total, a.batch_size))
        print('nchannels: ', data.channels_in)
        print('nsources: ', data.channels_out // data.channels_in)
        trainer = StereoTrainer(params=params, batch_size=a.batch_size, time_context=a.time_context, feat_size=data.F,
                                seed=a.seed)
        gen = torch.Generator(device=trainer.ctx.device)
        gen.manual_seed(a.seed)

        def redraw():
            with trainer.ctx.stream_scope():
                r = torch.randn(trainer.rand_shape, generator=gen, device=trainer.ctx.device, dtype=torch.float32) * RAND_STD
            trainer.set_rand(r)

        losser = []
        n = data.iteration_size
        epochs_done = [0]        # through the stages: the seed of the next epoch's window order

        def mse_stage(path, label, record):
            """--nepochs_mse epochs of train_fn_mse + train_fn1 (:238-260, :303-324), ``path`` saved after each."""
            for epoch in range(a.nepochs_mse):
                start_time = time.time()
                err = 0.0
                errs = np.zeros((data.channels_in, len(SOURCES)))
                for inputs, targets in data.batches(epochs_done[0]):
                    redraw()
                    err += trainer.step(inputs, targets)              # train_fn_mse (:204)
                    errs += trainer.losses(inputs, targets)           # train_fn1 (:206)
                epochs_done[0] += 1
                print("Epoch {} of {} took {:.3f}s".format(epoch + 1, a.nepochs_mse, time.time() - start_time))
                print("  training loss:\t\t{:.6f}".format(err / n))
                for j in range(errs.shape[0]):
                    for i, s in enumerate(SOURCES):
                        print("  training loss for " + s + " in mic " + str(j) + ":\t\t{:.6f}".format(errs[j][i] / n))
                print(label, path)
                trainer.save_model(path)
                if record:
                    losser.append(err / n)
            if a.nepochs_mse < 1:
                trainer.save_model(path)

        mse_state = None
        if not a.skip_train_mse:
            print("1st MSE training stage...")
            mse_stage(model_noILD, 'model_noILD: ', True)
            mse_state = trainer.optimizer_state()    # what train_fn_mse's updates (:202-204) hold when stage 3 calls it
        if not a.skip_train_ILD:
            if not a.skip_train_mse:
                trainer.set_params(load_model(model_noILD))           # :266-267
            trainer.set_optimizer('adadelta')                         # :269: a new adadelta, zero accumulators
            print("ILD training stage...")
            for epoch in range(a.nepochs_ILD):
                start_time = time.time()
                err = 0.0
                for inputs, targets in data.batches(epochs_done[0]):
                    redraw()
                    err += trainer.step(inputs, targets, ild=True)    # train_fn_ILD (:270)
                epochs_done[0] += 1
                print("Epoch {} of {} took {:.3f}s".format(epoch + 1, a.nepochs_ILD, time.time() - start_time))
                print("  training loss:\t\t{:.6f}".format(err / n))
                print('model_ILD: ', model_ILD)
                trainer.save_model(model_ILD)
                losser.append(err / n)
            if a.nepochs_ILD < 1:
                trainer.save_model(model_ILD)
        if not a.skip_train_mse:
            print("2nd MSE training stage...")
            trainer.set_params(load_model(model_ILD))                 # :298-299
            trainer.load_optimizer_state(mse_state)                   # :301's adadelta is never compiled: stage 1's state
            mse_stage(model_ILD_extra_mse, 'model_ILD_extra_mse: ', False)
        with open(os.path.join(output, 'models', "loss_" + name + ".data"), 'wb') as f:
            pickle.dump(losser, f, protocol=2)
        params = trainer.params()
        trainer.close()
    if not a.skip_sep:
        print("Separating")
        separate_all(params, db, os.path.join(output, 'output', name), a.scale_factor_test, a.time_context, a.overlap,
                     a.batch_size, mix_type='binaural' if a.binaural else 'mixture', mwf_iters=a.mwf)


if __name__ == "__main__":
    main()

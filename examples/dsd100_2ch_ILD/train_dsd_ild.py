#!/usr/bin/env python3
"""Train the stereo (ILD) DSD100 network on the MI355X: port of train_auto and __main__ of the reference's
examples/dsd100_2ch_ILD/trainCNN_ILD_DSD100.py.

    python train_dsd_ild.py --db <DSD100 root> --output <dir> [--feature_path F] [--model NAME] [--batch_size 32]
                            [--time_context 30] [--overlap 25] [--nepochs 30] [--scale_factor 0.3]
                            [--scale_factor_test 0.3] [--load] [--skip] [--skip_sep] [--seed 0] [--windows reference|all]
                            [--mwf N]

Features come from compute_features.py (``<feature_path>/*_in_m_.data`` / ``*_out_m_.data``, default
<db>/transforms/feature_folder).

Stage 1 (mse) runs --nepochs epochs of train_fn_mse + train_fn1, prints the reference's lines and saves
<output>/models/model_<NAME>_noILD.pkl after each.  Stage 2 (ILD) runs int(nepochs / 2) epochs of train_fn_ILD on a NEW
trainer loaded from the _noILD model -- the reference rebuilds ``adadelta`` there, which gives fresh accumulators -- and saves
<output>/models/model_<NAME>.pkl.  The loss list (both stages) is pickled as <output>/models/loss_<NAME>.data.  Then, unless
--skip_sep, Mixtures/{Dev,Test} are separated into <output>/output/<NAME>/Sources/<sub>/<song>/<source>.wav, stereo files.
--mwf N (default 0: the reference's block) puts N iterations of the multichannel Wiener filter between the network and the
inverse transform (the filter util.py:633-719 left unfinished; ``Separator.separate_stereo(audio, mwf_iters=N)``).

--load starts stage 1 from model_<NAME>_noILD.pkl if it is there, else from model_<NAME>.pkl; --skip trains nothing and
separates with model_<NAME>.pkl.

Differences from the reference: the two normal draws of the loss are replaced before every step from a device generator
seeded with --seed (Theano's RandomStreams(128) stream is not reproduced); the window order of an epoch is RandomState(seed
+ epoch).permutation (the reference's shuffle is unseeded); the scale factors are floats (the reference's int() of them is
a bug); --windows all takes every full window instead of the first getNum(T) ones that LargeDatasetMulti fills.
"""
import argparse
import os
import pickle
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd.separation import Separator, load_model, read_wav, write_wav  # noqa: E402
from deepconvsep_amd.stereo_training import RAND_STD, SOURCES, StereoFeatureWindows, StereoTrainer  # noqa: E402


def separate_all(params, db, outdir, scale_factor, tc, overlap, batch_size, mix_type='mixture', mwf_iters=0):
    """trainCNN_ILD_DSD100.py:291-341 with the fused stereo separation path; ``mix_type``: the file of each song that is
    separated, <mix_type>.wav (trainCNN_ILD_DSD100_3stages.py:543-546 and :335: 'binaural' for the binaural mixtures)."""
    sep = Separator('dsd_ild', params, scale_factor, tc, overlap, batch_size, 513, 1024, 512, np.hanning)
    for sub in ('Dev', 'Test'):
        d = os.path.join(db, 'Mixtures', sub)
        if not os.path.isdir(d):
            continue
        for song in sorted(os.listdir(d)):
            if song.startswith('.'):
                continue
            sampleRate, audio = read_wav(os.path.join(d, song, mix_type + '.wav'))
            assert sampleRate == 44100, "Sample rate needs to be 44100"
            if audio.ndim == 1:
                audio = np.repeat(audio[:, None], 2, axis=1)
            out = sep.separate_stereo(audio[:, :2], mwf_iters=mwf_iters)  # [L, S, 2]
            dirout = os.path.join(outdir, 'Sources', sub, song)
            os.makedirs(dirout, exist_ok=True)
            for i, s in enumerate(SOURCES):
                write_wav(os.path.join(dirout, s + '.wav'), out[:len(audio), i, :], sampleRate)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True)
    ap.add_argument("--output", required=True, help="the path where to save the model and the output")
    ap.add_argument("--feature_path")
    ap.add_argument("--model", default="model_name")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--time_context", type=int, default=30)
    ap.add_argument("--overlap", type=int, default=25)
    ap.add_argument("--nepochs", type=int, default=30)
    ap.add_argument("--scale_factor", type=float, default=0.3)
    ap.add_argument("--scale_factor_test", type=float, default=0.3)
    ap.add_argument("--load", action="store_true", help="start from the saved model")
    ap.add_argument("--skip", action="store_true", help="skip training")
    ap.add_argument("--skip_sep", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--windows", choices=("reference", "all"), default="reference")
    ap.add_argument("--mwf", type=int, default=0, help="iterations of the multichannel Wiener filter when separating")
    a = ap.parse_args(argv)
    db, output = a.db, a.output
    assert os.path.isdir(db), "Please input the directory for the DSD100 dataset with --db path_to_DSD100"
    assert os.path.isdir(output), "Please input the output directory --output path_to_output"
    os.makedirs(os.path.join(output, 'models'), exist_ok=True)
    model = os.path.join(output, 'models', "model_" + a.model + ".pkl")
    model_noILD = model[:-4] + '_noILD' + model[-4:]
    if a.skip:
        params = load_model(model)
    else:
        import torch
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
        params = None
        if a.load:
            params = load_model(model_noILD if os.path.isfile(model_noILD) else model)
        kw = dict(batch_size=a.batch_size, time_context=a.time_context, feat_size=data.F, seed=a.seed)
        trainer = StereoTrainer(params=params, **kw)
        gen = torch.Generator(device=trainer.ctx.device)
        gen.manual_seed(a.seed)

        def redraw(t):
            with t.ctx.stream_scope():
                r = torch.randn(t.rand_shape, generator=gen, device=t.ctx.device, dtype=torch.float32) * RAND_STD
            t.set_rand(r)

        losser = []
        n = data.iteration_size
        print("Training stage 1 (mse)...")
        for epoch in range(a.nepochs):
            start_time = time.time()
            err = 0.0
            errs = np.zeros((data.channels_in, len(SOURCES)))
            for inputs, targets in data.batches(epoch):
                redraw(trainer)
                err += trainer.step(inputs, targets)                  # train_fn_mse (:204)
                errs += trainer.losses(inputs, targets)               # train_fn1 (:206)
            print("Epoch {} of {} took {:.3f}s".format(epoch + 1, a.nepochs, time.time() - start_time))
            print("  training loss:\t\t{:.6f}".format(err / n))
            for j in range(errs.shape[0]):
                for i, s in enumerate(SOURCES):
                    print("  training loss for " + s + " in mic " + str(j) + ":\t\t{:.6f}".format(errs[j][i] / n))
            print('model_noILD: ', model_noILD)
            trainer.save_model(model_noILD)
            losser.append(err / n)
        if a.nepochs < 1:
            trainer.save_model(model_noILD)
        trainer.close()
        # :264-268: the parameters come back from the _noILD file and adadelta is rebuilt: a new trainer
        trainer = StereoTrainer(params=load_model(model_noILD), **kw)
        print("Training stage 2 (ILD)...")
        nild = int(a.nepochs / 2)
        for epoch in range(nild):
            start_time = time.time()
            err = 0.0
            for inputs, targets in data.batches(a.nepochs + epoch):
                redraw(trainer)
                err += trainer.step(inputs, targets, ild=True)        # train_fn_ILD (:268)
            print("Epoch {} of {} took {:.3f}s".format(epoch + 1, a.nepochs, time.time() - start_time))
            print("  training loss:\t\t{:.6f}".format(err / n))
            trainer.save_model(model)
            losser.append(err / n)
        if nild < 1:
            trainer.save_model(model)
        with open(os.path.join(output, 'models', "loss_" + a.model + ".data"), 'wb') as f:
            pickle.dump(losser, f, protocol=2)
        params = trainer.params()
        trainer.close()
    if not a.skip_sep:
        print("Separating")
        separate_all(params, db, os.path.join(output, 'output', a.model), a.scale_factor_test, a.time_context, a.overlap,
                     a.batch_size, mwf_iters=a.mwf)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Train the DSD100 separation network on the MI355X: port of the reference's examples/dsd100/trainCNN.py.

    python train_dsd.py --db <DSD100 root> [--feature_path F] [--model NAME] [--batch_size 32] [--time_context 30]
                        [--overlap 25] [--nepochs 40] [--scale_factor 0.3] [--load] [--skip_sep] [--seed 0]
                        [--windows reference|all]

Features come from compute_features.py (``<feature_path>/*.data``, default <db>/transforms/t1).  Per epoch the reference's
lines are printed and the model is saved as <db>/models/model_<NAME>.pkl (the format separate_dsd.py loads); the per-epoch
loss list is pickled as <db>/models/loss_<NAME>.data.  Then, unless --skip_sep, Mixtures/{Dev,Test} are separated into
<db>/output/<NAME>.  Differences from the reference: the window order of an epoch is RandomState(seed + epoch).permutation
(the reference's shuffle is unseeded); --scale_factor is a float (the reference's int() of it is a bug); --windows all takes
every full window instead of the first getNum(T) ones that LargeDataset fills.
"""
import argparse
import glob
import os
import pickle
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd.separation import Separator, blackmanharris, load_model, read_wav, write_wav  # noqa: E402
from deepconvsep_amd.training import FeatureWindows, Trainer  # noqa: E402

SOURCES = ['vocals', 'bass', 'drums', 'other']


def separate_all(params, testdir, outdir, scale_factor, tc, overlap, batch_size):
    """trainCNN.py:275-313 with the fused separation path."""
    sep = Separator('dsd', params, scale_factor, tc, overlap, batch_size, 513, 1024, 512, blackmanharris)
    for split in ("Dev", "Test"):
        d = os.path.join(testdir, split)
        if not os.path.isdir(d):
            continue
        for f in sorted(os.listdir(d)):
            if f.startswith('.'):
                continue
            sampleRate, audioObj = read_wav(os.path.join(d, f, "mixture.wav"))
            assert sampleRate == 44100, "Sample rate needs to be 44100"
            audio = (audioObj[:, 0] + audioObj[:, 1]) / 2 if audioObj.ndim > 1 else audioObj
            out = sep.separate(audio)
            dirout = os.path.join(outdir, split, f)
            os.makedirs(dirout, exist_ok=True)
            for i in range(out.shape[0]):
                write_wav(os.path.join(dirout, SOURCES[i] + '.wav'), out[i][:len(audio)], sampleRate)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True)
    ap.add_argument("--feature_path")
    ap.add_argument("--model", default="dsd_fft_1024")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--time_context", type=int, default=30)
    ap.add_argument("--overlap", type=int, default=25)
    ap.add_argument("--nepochs", type=int, default=40)
    ap.add_argument("--scale_factor", type=float, default=0.3)
    ap.add_argument("--load", action="store_true", help="resume from models/model_<model>.pkl")
    ap.add_argument("--skip_sep", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--windows", choices=("reference", "all"), default="reference")
    a = ap.parse_args(argv)
    db = a.db
    assert os.path.isdir(db), "Please input the directory for the DSD100 dataset with --db path_to_DSD100"
    feature_path = a.feature_path or os.path.join(db, 'transforms', 't1')
    paths = sorted(glob.glob(os.path.join(feature_path, "*.data")))
    if not paths:
        raise SystemExit("no .data feature files under %s: run compute_features.py first" % feature_path)
    data = FeatureWindows(paths, a.time_context, a.overlap, a.scale_factor, a.windows, a.batch_size, a.seed)
    if data.iteration_size == 0:
        raise SystemExit("%d windows are fewer than one batch of %d" % (data.total, a.batch_size))
    os.makedirs(os.path.join(db, 'models'), exist_ok=True)
    model = os.path.join(db, 'models', "model_" + a.model + ".pkl")
    params = load_model(model) if a.load else None
    trainer = Trainer(params=params, batch_size=a.batch_size, time_context=a.time_context, feat_size=data.F, seed=a.seed)
    losser = []
    for epoch in range(a.nepochs):
        start_time = time.time()
        err = 0.0
        comp = np.zeros(6)
        for inputs, targets in data.batches(epoch):
            err += trainer.step(inputs, targets)                 # train_fn (trainCNN.py:262)
            comp += np.asarray(trainer.losses(inputs, targets))  # train_fn1 (:263)
        n = data.iteration_size
        print("Epoch {} of {} took {:.3f}s".format(epoch + 1, a.nepochs, time.time() - start_time))
        print("  training loss:\t\t{:.6f}".format(err / n))
        print("  training loss for vocals:\t\t{:.6f}".format(comp[0] / n))
        print("  training loss for bass:\t\t{:.6f}".format(comp[1] / n))
        print("  training loss for drums:\t\t{:.6f}".format(comp[2] / n))
        print("  Beta component:\t\t{:.6f}".format(comp[3] / n))
        print("  Beta component for voice:\t\t{:.6f}".format(comp[5] / n))
        print("  alpha component:\t\t{:.6f}".format(comp[4] / n))
        losser.append(err / n)   # the reference appends each epoch's loss twice (trainCNN.py:289, :296)
        losser.append(err / n)
        trainer.save_model(model)
    with open(os.path.join(db, 'models', "loss_" + a.model + ".data"), 'wb') as f:
        pickle.dump(losser, f, protocol=2)
    if not a.skip_sep:
        separate_all(trainer.params(), os.path.join(db, 'Mixtures'), os.path.join(db, 'output', a.model), a.scale_factor,
                     a.time_context, a.overlap, a.batch_size)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Train the iKala singing-voice network on the MI355X: port of the reference's examples/ikala/trainCNN.py.

    python train_ikala.py --db <iKala root> [--feature_path F] [--model fft_1024] [--batch_size 32] [--time_context 30]
                          [--overlap 20] [--nepochs 40] [--scale_factor 0.3] [--load] [--skip_sep] [--seed 0]
                          [--windows reference|all]

Features come from compute_features.py (``<feature_path>/*.data``, default <db>/transforms/t1).  Per epoch the reference's
five lines are printed and the model is saved as <db>/models/model_<NAME>.pkl (the format separate_ikala.py loads); the
per-epoch loss list (one entry per epoch, trainCNN.py:243) is pickled as <db>/models/loss_<NAME>.data.  Then, unless
--skip_sep, every Wavfile/*.wav (mixture = left + right) is separated into <db>/output/<NAME>/<name>-voice.wav and
-music.wav.  Differences from the reference: the window order of an epoch is RandomState(seed + epoch).permutation (the
reference's shuffle is unseeded); --scale_factor is a float (the reference's int() of it is a bug); --windows all takes
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


def separate_all(params, testdir, outdir, scale_factor, tc, overlap, batch_size):
    """trainCNN.py:249-283 with the fused separation path."""
    sep = Separator('ikala', params, scale_factor, tc, overlap, batch_size, 513, 1024, 512, blackmanharris)
    os.makedirs(outdir, exist_ok=True)
    for f in sorted(os.listdir(testdir)):
        if not f.endswith(".wav"):
            continue
        sampleRate, audioObj = read_wav(os.path.join(testdir, f))
        assert sampleRate == 44100, "Sample rate needs to be 44100"
        audio = audioObj[:, 0] + audioObj[:, 1]
        out = sep.separate(audio)
        write_wav(os.path.join(outdir, f.replace(".wav", "-voice.wav")), out[0][:len(audio)], sampleRate)
        write_wav(os.path.join(outdir, f.replace(".wav", "-music.wav")), out[1][:len(audio)], sampleRate)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True)
    ap.add_argument("--feature_path")
    ap.add_argument("--model", default="fft_1024")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--time_context", type=int, default=30)
    ap.add_argument("--overlap", type=int, default=20)
    ap.add_argument("--nepochs", type=int, default=40)
    ap.add_argument("--scale_factor", type=float, default=0.3)
    ap.add_argument("--load", action="store_true", help="resume from models/model_<model>.pkl")
    ap.add_argument("--skip_sep", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--windows", choices=("reference", "all"), default="reference")
    a = ap.parse_args(argv)
    db = a.db
    assert os.path.isdir(db), "Please input the directory for the iKala dataset with --db path_to_iKala"
    feature_path = a.feature_path or os.path.join(db, 'transforms', 't1')
    paths = sorted(glob.glob(os.path.join(feature_path, "*.data")))
    if not paths:
        raise SystemExit("no .data feature files under %s: run compute_features.py first" % feature_path)
    data = FeatureWindows(paths, a.time_context, a.overlap, a.scale_factor, a.windows, a.batch_size, a.seed, sources=2)
    if data.iteration_size == 0:
        raise SystemExit("%d windows are fewer than one batch of %d" % (data.total, a.batch_size))
    os.makedirs(os.path.join(db, 'models'), exist_ok=True)
    model = os.path.join(db, 'models', "model_" + a.model + ".pkl")
    params = load_model(model) if a.load else None
    trainer = Trainer(arch='ikala_nopool', params=params, batch_size=a.batch_size, time_context=a.time_context,
                      feat_size=data.F, seed=a.seed)
    losser = []
    for epoch in range(a.nepochs):
        start_time = time.time()
        err = 0.0
        comp = np.zeros(4)
        for inputs, targets in data.batches(epoch):
            err += trainer.step(inputs, targets)                 # train_fn (trainCNN.py:228)
            comp += np.asarray(trainer.losses(inputs, targets))  # train_fn1 (:229)
        n = data.iteration_size
        print("Epoch {} of {} took {:.3f}s".format(epoch + 1, a.nepochs, time.time() - start_time))
        print("  training loss:\t\t{:.6f}".format(err / n))
        print("  training loss for vocals:\t\t{:.6f}".format(comp[0] / n))
        print("  training loss for acc:\t\t{:.6f}".format(comp[1] / n))
        print("  Beta component for voice:\t\t{:.6f}".format(comp[2] / n))
        print("  Beta component for acc:\t\t{:.6f}".format(comp[3] / n))
        losser.append(err / n)
        trainer.save_model(model)
    with open(os.path.join(db, 'models', "loss_" + a.model + ".data"), 'wb') as f:
        pickle.dump(losser, f, protocol=2)
    if not a.skip_sep:
        separate_all(trainer.params(), os.path.join(db, 'Wavfile'), os.path.join(db, 'output', a.model), a.scale_factor,
                     a.time_context, a.overlap, a.batch_size)


if __name__ == "__main__":
    main()

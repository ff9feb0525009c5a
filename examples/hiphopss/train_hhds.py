#!/usr/bin/env python3
"""Train the hiphop (HHDS) separation network on the MI355X: port of the reference's examples/hiphopss/trainCNN.py and
augmentations/trainCNN_{cs,instr,mix}_aug.py.

    python train_hhds.py --db <HHDS root> [--augment none|cs|instr|mix] [--render] [--feature_path F] [--model NAME]
                         [--batch_size 32] [--time_context 30] [--overlap 25] [--nepochs 40] [--scale_factor 0.3] [--load]
                         [--skip_sep] [--seed 0] [--windows reference|all]

The network and the loss are the DSD100 ones (the four reference trainers differ from examples/dsd100/trainCNN.py in paths
and names).  --augment selects the feature path (<db>/transforms/t1, t1_cs_aug, t1_instr_aug, t1_mix_aug) and the model
name (hh_fft_1024, hh_cs_aug_fft_1024, hh_instr_aug_fft_1024, hh_mix_aug_fft_1024); 'mix' trains with alpha, beta and
beta_voc at a thousandth (trainCNN_mix_aug.py:164-166); 'instr' separates Dev/<song>/mixture_5.wav
(trainCNN_instr_aug.py:292).  Without --render the ``.data`` files of compute_features.py are read (FeatureWindows, as
train_dsd.py); with --render there are no feature files: the sources' wav files go to the device once and every batch of
windows is transformed from them, augmentation included (RenderedWindows, dcs_trainer_gather_render).  Differences from the
reference: those of examples/dsd100/train_dsd.py; mono mixtures are accepted as in trainCNN.py:299-302.
"""
import argparse
import glob
import os
import pickle
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd import augment  # noqa: E402
from deepconvsep_amd.separation import Separator, blackmanharris, load_model, read_wav, write_wav  # noqa: E402
from deepconvsep_amd.training import ALPHA, BETA, BETA_VOC, FeatureWindows, Trainer  # noqa: E402

SOURCES = ['vocals', 'bass', 'drums', 'other']
FEATURE_DIRS = {'none': 't1', 'cs': 't1_cs_aug', 'instr': 't1_instr_aug', 'mix': 't1_mix_aug'}
MODELS = {'none': 'hh_fft_1024', 'cs': 'hh_cs_aug_fft_1024', 'instr': 'hh_instr_aug_fft_1024', 'mix': 'hh_mix_aug_fft_1024'}


def loss_weights(kind):
    """alpha, beta, beta_voc: trainCNN.py:167-170; a thousandth of them for mix_aug (trainCNN_mix_aug.py:162-166)."""
    return (0.000001, 0.00001, 0.00003) if kind == 'mix' else (ALPHA, BETA, BETA_VOC)


def dev_mixture(kind):
    return "mixture_5.wav" if kind == 'instr' else "mixture.wav"


def separate_all(params, testdir, outdir, scale_factor, tc, overlap, batch_size, kind, frame, hop):
    """trainCNN.py:279-336 with the fused separation path."""
    sep = Separator('hiphop', params, scale_factor, tc, overlap, batch_size, frame // 2 + 1, frame, hop, blackmanharris)
    for split in ("Dev", "Test"):
        d = os.path.join(testdir, split)
        if not os.path.isdir(d):
            continue
        for f in sorted(os.listdir(d)):
            if f.startswith('.'):
                continue
            sampleRate, audioObj = read_wav(os.path.join(d, f, dev_mixture(kind) if split == "Dev" else "mixture.wav"))
            if audioObj.ndim > 1 and audioObj.shape[1] > 1:
                audio = (audioObj[:, 0] + audioObj[:, 1]) / 2
            else:                                                    # mono (trainCNN.py:299-302)
                audio = audioObj[:, 0] if audioObj.ndim > 1 else audioObj
            out = sep.separate(audio)
            dirout = os.path.join(outdir, split, f)
            os.makedirs(dirout, exist_ok=True)
            for i in range(out.shape[0]):
                write_wav(os.path.join(dirout, SOURCES[i] + '.wav'), out[i][:len(audio)], sampleRate)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True)
    ap.add_argument("--augment", choices=augment.KINDS, default="none")
    ap.add_argument("--render", action="store_true", help="train from the wav files: no feature files are read or written")
    ap.add_argument("--feature_path")
    ap.add_argument("--model")
    ap.add_argument("--batch_size", type=int, default=32)
    ap.add_argument("--time_context", type=int, default=30)
    ap.add_argument("--overlap", type=int, default=25)
    ap.add_argument("--nepochs", type=int, default=40)
    ap.add_argument("--scale_factor", type=float, default=0.3)
    ap.add_argument("--load", action="store_true", help="resume from models/model_<model>.pkl")
    ap.add_argument("--skip_sep", action="store_true")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--windows", choices=("reference", "all"), default="reference")
    ap.add_argument("--frameSize", type=int, default=1024)
    ap.add_argument("--hopSize", type=int, default=512)
    ap.add_argument("--sample_rate", type=int, default=44100)
    ap.add_argument("--chunk", type=int, help="--render: samples per chunk (default 30 s)")
    a = ap.parse_args(argv)
    db = a.db
    assert os.path.isdir(db), "Please input the directory for the dataset with --db path"
    name = a.model or MODELS[a.augment]
    if a.render:
        signals, vfiles, _ = augment.dataset_signals(db, a.augment, a.sample_rate, a.chunk, a.seed)
        data = augment.RenderedWindows(signals, vfiles, a.time_context, a.overlap, a.scale_factor, a.windows, a.batch_size,
                                       a.seed, frameSize=a.frameSize, hopSize=a.hopSize, window=blackmanharris)
    else:
        feature_path = a.feature_path or os.path.join(db, 'transforms', FEATURE_DIRS[a.augment])
        paths = sorted(glob.glob(os.path.join(feature_path, "*.data")))
        if not paths:
            raise SystemExit("no .data feature files under %s: run compute_features.py --augment %s first, or train with "
                             "--render" % (feature_path, a.augment))
        data = FeatureWindows(paths, a.time_context, a.overlap, a.scale_factor, a.windows, a.batch_size, a.seed)
    if data.iteration_size == 0:
        raise SystemExit("%d windows are fewer than one batch of %d" % (data.total, a.batch_size))
    os.makedirs(os.path.join(db, 'models'), exist_ok=True)
    model = os.path.join(db, 'models', "model_" + name + ".pkl")
    params = load_model(model) if a.load else None
    alpha, beta, beta_voc = loss_weights(a.augment)
    trainer = Trainer(params=params, batch_size=a.batch_size, time_context=a.time_context, feat_size=data.F, seed=a.seed,
                      alpha=alpha, beta=beta, beta_voc=beta_voc)
    losser = []
    for epoch in range(a.nepochs):
        start_time = time.time()
        err = 0.0
        comp = np.zeros(6)
        for inputs, targets in data.batches(epoch):
            err += trainer.step(inputs, targets)                 # train_fn (trainCNN.py:224)
            comp += np.asarray(trainer.losses(inputs, targets))  # train_fn1 (:225)
        n = data.iteration_size
        print("Epoch {} of {} took {:.3f}s".format(epoch + 1, a.nepochs, time.time() - start_time))
        print("  training loss:\t\t{:.6f}".format(err / n))
        print("  training loss for vocals:\t\t{:.6f}".format(comp[0] / n))
        print("  training loss for bass:\t\t{:.6f}".format(comp[1] / n))
        print("  training loss for drums:\t\t{:.6f}".format(comp[2] / n))
        print("  Beta component:\t\t{:.6f}".format(comp[3] / n))
        print("  Beta component for voice:\t\t{:.6f}".format(comp[5] / n))
        print("  alpha component:\t\t{:.6f}".format(comp[4] / n))
        losser.append(err / n)   # the reference appends each epoch's loss twice, as dsd100/trainCNN.py does
        losser.append(err / n)
        trainer.save_model(model)
    with open(os.path.join(db, 'models', "loss_" + name + ".data"), 'wb') as f:
        pickle.dump(losser, f, protocol=2)
    if not a.skip_sep:
        separate_all(trainer.params(), os.path.join(db, 'Mixtures'), os.path.join(db, 'output', name), a.scale_factor,
                     a.time_context, a.overlap, a.batch_size, a.augment, a.frameSize, a.hopSize)


if __name__ == "__main__":
    main()

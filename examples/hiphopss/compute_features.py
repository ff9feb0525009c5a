#!/usr/bin/env python3
"""Port of the reference's examples/hiphopss/compute_features.py and augmentations/compute_features_{cs,instr,mix}_aug.py:
the training features of the hiphop (HHDS) data set on the MI355X.

    python compute_features.py --db <HHDS root> [--augment none|cs|instr|mix] [--feature_path <out dir>] [--seed 0]

One ``[5, T, 513]`` float64 magnitude tensor (mixture, vocals, bass, drums, other) per 30 s chunk and for the rest of the
file, ``<name>__m_.data`` / ``.shape`` as ``transformFFT(1024, 512, blackmanharris).compute_transform`` writes them, under
<db>/transforms/t1, t1_cs_aug, t1_instr_aug or t1_mix_aug.  The variants are not rendered on the host: the sources of a song
go to the device once and every variant -- shifted, muted, mixed across songs -- is formed inside the STFT's loader, all
chunks of a variant in one launch (deepconvsep_amd.augment.render_features, dcs_stft_forward_render_f64).

none   <song>_<i>; writes Mixtures/Dev/<song>/mixture.wav if it is missing (compute_features.py:96-99)
cs     14 shift patterns of (0, 0.2 s) per source; <song>_<i>_cs<0/1 per source: vocals, bass, drums, other> -- the
       reference pastes NumPy's array repr into the name, which depends on the NumPy version
instr  one source muted (1 .. 4) or none (5), mixture / 4; <song>_<i>_<ins>; writes mixture_<ins>.wav
mix    every song with mixture / 4 (writes mixture.wav), then the four sources from four different songs for every tenth
       combination and permutation, drawn from --seed (unseeded in the reference); combination_<c>_perm_<p>_block_<i>

A song shorter than 30 s gives its rest chunk only.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", ".."))

from deepconvsep_amd import augment  # noqa: E402
from deepconvsep_amd.separation import blackmanharris, write_wav  # noqa: E402
from deepconvsep_amd.transform import transformFFT  # noqa: E402

FEATURE_DIRS = {'none': 't1', 'cs': 't1_cs_aug', 'instr': 't1_instr_aug', 'mix': 't1_mix_aug'}


def mixture_wav(kind, song, index):
    """The wav the reference's generator writes next to the song's mixture for its ``index``-th virtual file (None: none)."""
    if kind == 'instr':
        return 'mixture_%d.wav' % (index + 1)
    return 'mixture.wav' if kind in ('none', 'mix') and song is not None else None


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--db", required=True, help="the dataset path")
    ap.add_argument("--augment", choices=augment.KINDS, default="none")
    ap.add_argument("--feature_path", help="the path where to save the features (default <db>/transforms/t1[_<augment>_aug])")
    ap.add_argument("--seed", type=int, default=0, help="mix: the draws that pick every tenth combination / permutation")
    ap.add_argument("--frameSize", type=int, default=1024)
    ap.add_argument("--hopSize", type=int, default=512)
    ap.add_argument("--sample_rate", type=int, default=44100)
    ap.add_argument("--chunk", type=int, help="samples per chunk (default 30 s)")
    a = ap.parse_args(argv)
    db = a.db
    assert os.path.isdir(db), "Please input the directory for the dataset with --db path"
    feature_path = a.feature_path or os.path.join(db, 'transforms', FEATURE_DIRS[a.augment])
    signals, _, songs = augment.dataset_signals(db, a.augment, a.sample_rate, a.chunk, a.seed)
    tt = transformFFT(frameSize=a.frameSize, hopSize=a.hopSize, sampleRate=a.sample_rate, window=blackmanharris)
    bank, bank_keys = None, None
    for song, split, vfiles in songs:
        n = 0
        for index, vf in enumerate(vfiles):
            keys = sorted(set(t.signal for t in vf.tracks))
            if keys != bank_keys:            # a song's variants share its four sources: one upload
                bank, bank_keys = augment.Bank({k: signals[k] for k in keys}, np.float64, tt._get_plan().ctx), keys
            n += len(augment.render_features(tt, bank, vf, feature_path))
            wav = mixture_wav(a.augment, song, index)
            if wav is not None:
                out = os.path.join(db, "Mixtures", split, song, wav)
                if a.augment != 'none' or not os.path.isfile(out):
                    write_wav(out, augment.render_audio(signals, vf)[0], a.sample_rate)
        print("features of %s: %d files" % (song if song is not None else "the mixed songs", n))


if __name__ == "__main__":
    main()

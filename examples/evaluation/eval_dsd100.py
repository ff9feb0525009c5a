#!/usr/bin/env python3
"""DSD100 scores on one MI355X: the arithmetic of the reference's evaluation/DSD100_eval_only.m, without a cluster.

    python eval_dsd100.py <dataset_folder> <estimates_folder> [-o results.json] [--subset Dev|Test] [--song NAME]

References: <dataset_folder>/Sources/<Dev|Test>/<song>/{bass,drums,other,vocals}.wav.  Estimates:
<estimates_folder>/<Dev|Test>/<song>/<source>.wav (the names separate_dsd.py writes) or mixture_<source>.wav (the MATLAB
script's names, 'mixture_others' for other); an optional accompaniment estimate (accompaniment.wav or
mixture_accompaniment.wav) replaces the sum of the first three estimates.  A missing estimate is silence.  Mono channels
are duplicated to stereo, every signal is cut to the shortest estimate, and the framewise bss_eval (30 s windows, 15 s hop,
512-tap filters) runs on the four sources and on vocals / accompaniment.  The JSON holds, per song, the per-window
SDR / ISR / SIR / SAR and their NaN-ignoring medians (the SiSEC summary).
"""
import argparse
import os

import numpy as np

from common import dump, find, metrics, read

from deepconvsep_amd.evaluation import FLEN, bss_eval  # noqa: E402

SOURCES = ["bass", "drums", "other", "vocals"]
MATLAB_NAMES = {"bass": "mixture_bass", "drums": "mixture_drums", "other": "mixture_others", "vocals": "mixture_vocals"}
KEYS = ("SDR", "ISR", "SIR", "SAR")


def stereo(x):
    return np.repeat(x, 2, axis=1) if x.shape[1] == 1 else x[:, :2]


def evaluate_song(src_dir, est_dir, win_s=30, hop_s=15, flen=FLEN):
    refs, rate = [], None
    for s in SOURCES:
        rate, x = read(os.path.join(src_dir, s + ".wav"))
        refs.append(stereo(x))
    n = min(len(x) for x in refs)
    ests = [None] * 4
    for q, s in enumerate(SOURCES):
        p = find(est_dir, [s + ".wav", MATLAB_NAMES[s] + ".wav"])
        if p:
            ests[q] = stereo(read(p)[1])
            n = min(n, len(ests[q]))
    acc_path = find(est_dir, ["accompaniment.wav", "mixture_accompaniment.wav"])
    acc_est = stereo(read(acc_path)[1]) if acc_path else None
    if acc_est is not None:
        n = min(n, len(acc_est))
    ests = [np.zeros((n, 2)) if e is None else e[:n] for e in ests]
    refs = [r[:n] for r in refs]
    i = np.stack(refs, axis=2)                                  # [nsampl, nchan, nsrc]
    ie = np.stack(ests, axis=2)
    acc_ref = i[:, :, :3].sum(axis=2)
    acc_est = ie[:, :, :3].sum(axis=2) if acc_est is None else acc_est[:n]
    win, hop = win_s * rate, hop_s * rate
    four = dict(zip(KEYS, bss_eval(ie, i, win, hop, flen)))
    two = dict(zip(KEYS, bss_eval(np.stack([ie[:, :, 3], acc_est], axis=2), np.stack([i[:, :, 3], acc_ref], axis=2),
                                  win, hop, flen)))
    res = metrics(SOURCES, four, KEYS)
    res["accompaniment"] = metrics(["vocals", "accompaniment"], two, KEYS)["accompaniment"]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("dataset_folder")
    ap.add_argument("estimates_folder")
    ap.add_argument("-o", "--out", default=None, help="JSON file (default: stdout)")
    ap.add_argument("--subset", choices=["Dev", "Test"], action="append", help="default: both")
    ap.add_argument("--song", action="append", help="only these songs")
    ap.add_argument("--win", type=int, default=30, help="window, seconds (30)")
    ap.add_argument("--hop", type=int, default=15, help="hop, seconds (15)")
    ap.add_argument("--flen", type=int, default=FLEN)
    a = ap.parse_args(argv)
    out = {}
    for subset in a.subset or ["Test", "Dev"]:
        sdir = os.path.join(a.dataset_folder, "Sources", subset)
        if not os.path.isdir(sdir):
            continue
        for song in sorted(os.listdir(sdir)):
            if a.song and song not in a.song:
                continue
            out.setdefault(subset, {})[song] = evaluate_song(os.path.join(sdir, song),
                                                             os.path.join(a.estimates_folder, subset, song),
                                                             a.win, a.hop, a.flen)
    dump(out, a.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Bach10 scores on one MI355X: the arithmetic of the reference's evaluation/Bach10_eval_only.m.

    python eval_bach10.py <dataset_folder> <estimates_folder> [-o results.json]

References: <dataset_folder>/Sources/<song>/<song>-<instrument>.wav; estimates: <estimates_folder>/<song>-<instrument>.wav
(or <song>_<instrument>.wav, the names separate_bach10.py writes).  A missing estimate is silence; every signal is cut to
the shortest estimate.  bss_eval_sources over the four instruments (512-tap filters, best permutation: ``perm`` in the
JSON is 0-based, estimate perm[j] goes with instrument j).
"""
import argparse
import os

import numpy as np

from common import dump, find, metrics, read

from deepconvsep_amd.evaluation import FLEN, bss_eval_sources  # noqa: E402

INSTRUMENTS = ["bassoon", "clarinet", "saxphone", "violin"]


def mono(x):
    return x.mean(axis=1)


def evaluate_song(src_dir, est_dir, song, flen=FLEN):
    refs = [mono(read(os.path.join(src_dir, "%s-%s.wav" % (song, s)))[1]) for s in INSTRUMENTS]
    n = min(len(r) for r in refs)
    ests = []
    for s in INSTRUMENTS:
        p = find(est_dir, ["%s-%s.wav" % (song, s), "%s_%s.wav" % (song, s)])
        ests.append(mono(read(p)[1]) if p else None)
        if p:
            n = min(n, len(ests[-1]))
    est = np.stack([np.zeros(n) if e is None else e[:n] for e in ests])
    sdr, sir, sar, perm = bss_eval_sources(est, np.stack([r[:n] for r in refs]), flen)
    res = metrics(INSTRUMENTS, {"SDR": sdr, "SIR": sir, "SAR": sar}, ("SDR", "SIR", "SAR"))
    res["perm"] = [int(p) for p in perm]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("dataset_folder")
    ap.add_argument("estimates_folder")
    ap.add_argument("-o", "--out", default=None, help="JSON file (default: stdout)")
    ap.add_argument("--flen", type=int, default=FLEN)
    a = ap.parse_args(argv)
    sdir = os.path.join(a.dataset_folder, "Sources")
    out = {song: evaluate_song(os.path.join(sdir, song), a.estimates_folder, song, a.flen)
           for song in sorted(os.listdir(sdir)) if os.path.isdir(os.path.join(sdir, song))}
    dump(out, a.out)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""iKala scores on one MI355X: the arithmetic of the reference's evaluation/evaluate_SS_iKala.m.

    python eval_ikala.py <Wavfile folder> <estimates folder> [-o results.json]

For every <name>.wav of the dataset (left channel = music, right = voice) the estimates <name>-voice.wav and
<name>-music.wav (the names separate_ikala.py writes) are read, cut to the shortest signal, and both sides divided by
the norm of their sum; bss_eval_sources (512-tap filters, best permutation) gives SDR / SIR / SAR, and the same call with
the mixture (voice + music) / 2 as both estimates gives the normalised NSDR / NSIR / NSAR = SDR - SDR(mixture) etc.
"""
import argparse
import os

import numpy as np

from common import dump, metrics, read

from deepconvsep_amd.evaluation import FLEN, bss_eval_sources  # noqa: E402

NAMES = ["voice", "music"]


def evaluate_file(wav, est_dir, flen=FLEN):
    base = os.path.basename(wav)
    x = read(wav)[1]
    true_voice, true_music = x[:, 1], x[:, 0]
    ev = read(os.path.join(est_dir, base.replace(".wav", "-voice.wav")))[1][:, 0]
    em = read(os.path.join(est_dir, base.replace(".wav", "-music.wav")))[1][:, 0]
    n = min(len(true_voice), len(ev), len(em))
    true = np.stack([true_voice[:n], true_music[:n]])
    est = np.stack([ev[:n], em[:n]])
    mix = (true[0] + true[1]) / 2
    mixed = np.stack([mix, mix])
    true_n = true / np.linalg.norm(true[0] + true[1])
    sdr, sir, sar, perm = bss_eval_sources(est / np.linalg.norm(est[0] + est[1]), true_n, flen)
    msdr, msir, msar, _ = bss_eval_sources(mixed / np.linalg.norm(mixed[0] + mixed[1]), true_n, flen)
    vals = {"SDR": sdr, "SIR": sir, "SAR": sar, "NSDR": sdr - msdr, "NSIR": sir - msir, "NSAR": sar - msar}
    res = metrics(NAMES, vals, tuple(vals))
    res["perm"] = [int(p) for p in perm]
    return res


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("wav_folder")
    ap.add_argument("estimates_folder")
    ap.add_argument("-o", "--out", default=None, help="JSON file (default: stdout)")
    ap.add_argument("--flen", type=int, default=FLEN)
    a = ap.parse_args(argv)
    out = {}
    for name in sorted(os.listdir(a.wav_folder)):
        if not name.endswith(".wav"):
            continue
        if not os.path.isfile(os.path.join(a.estimates_folder, name.replace(".wav", "-voice.wav"))):
            continue                                  # as the script: only files with an estimate
        out[name[:-4]] = evaluate_file(os.path.join(a.wav_folder, name), a.estimates_folder, a.flen)
    dump(out, a.out)


if __name__ == "__main__":
    main()
